"""Float-free restatement of the class location tables (csrc/locations.hip, utils.data.class_locations) and of the foreground draw
(utils.data.foreground_origin), written without looking at either: plain Python integers, a loop over regions and over j.

  label   uint8 [S0, S1, S2], linear index v in C order.  Values 0..4 are classes, 4 read as 3; anything else belongs to no region.
  region  r holds class c iff (posmasks[r] >> c) & 1; 1 <= R <= 8, regions may overlap.
  counts  counts[r] = n_r, the voxels of region r.
  table   m_r = min(n_r, K); table[r][j] = the region voxel of rank (j * n_r) // m_r for j < m_r (rank 0 = smallest linear index),
          -1 for j >= m_r.
  draw    stream default_rng([seed, epoch, index, 1]): u = random(); foreground iff u < oversample and some n_r > 0; then
          r = the integers(0, #non-empty)-th non-empty region, j = integers(0, m_r), v = unravel(table[r][j]),
          origin_d = clamp(v_d - crop_d // 2, 0, max(S_d - crop_d, 0)).
"""
import numpy as np

FOREGROUND_CLASSES = (0b0010, 0b0100, 0b1000)


def region_voxels(label, posmask):
    """the linear indices of one region, increasing (int64)"""
    flat = np.asarray(label, dtype=np.uint8).reshape(-1)
    out = [np.zeros(0, dtype=np.int64)]
    for c in range(4):
        if (int(posmask) >> c) & 1:
            out.append(np.nonzero(flat == c)[0])
            if c == 3:
                out.append(np.nonzero(flat == 4)[0])
    return np.sort(np.concatenate(out).astype(np.int64))


def class_locations(label, posmasks=FOREGROUND_CLASSES, K=4096):
    """(counts int64 [R], table int32 [R, K])"""
    K = int(K)
    counts = np.zeros(len(posmasks), dtype=np.int64)
    table = np.empty((len(posmasks), K), dtype=np.int32)
    for r, mask in enumerate(posmasks):
        vox = region_voxels(label, mask)
        n = len(vox)
        m = min(n, K)
        counts[r] = n
        for j in range(K):
            table[r, j] = vox[(j * n) // m] if j < m else -1
    return counts, table


def foreground_origin(seed, epoch, index, full, crop, counts, table, oversample):
    """(origin, r, v) or (None, None, None)"""
    rng = np.random.default_rng([int(seed), int(epoch), int(index), 1])
    u = float(rng.random())
    present = []
    for r in range(len(counts)):
        if int(counts[r]) > 0:
            present.append(r)
    if not (u < oversample) or not present:
        return None, None, None
    r = present[int(rng.integers(0, len(present)))]
    m = min(int(counts[r]), int(np.asarray(table).shape[1]))
    lin = int(table[r][int(rng.integers(0, m))])
    s0, s1, s2 = (int(s) for s in full)
    v = (lin // (s1 * s2), (lin // s2) % s1, lin % s2)
    origin = []
    for d in range(3):
        o = v[d] - int(crop[d]) // 2
        hi = max(int(full[d]) - int(crop[d]), 0)
        origin.append(0 if o < 0 else hi if o > hi else o)
    return tuple(origin), r, v


def region_classes(posmask):
    """the label values (after 4 -> 3) of a region"""
    return [c for c in range(4) if (int(posmask) >> c) & 1]


# ------------------------------------------------------------------------------------------------------------------ test labels
OVERLAPPING = (0b1110, 0b1010, 0b1000)                                            # WT / TC / ET
EIGHT = (0b0001, 0b0010, 0b0100, 0b1000, 0b1110, 0b1010, 0b0110, 0b0000)          # R = 8, one region that holds no class


def label_families(shape, tile, seed=0):
    """{name: uint8 label of `shape`}: the label families of the location-table tests.  `tile` is the kernel's tile size: single voxels
    sit on both sides of a tile edge where the volume reaches it."""
    shape = tuple(int(s) for s in shape)
    V = int(np.prod(shape))
    rng = np.random.default_rng([seed, V])
    fam = {"background": np.zeros(V, dtype=np.uint8), "one_class": np.full(V, 2, dtype=np.uint8)}
    for name, at in (("first", 0), ("last", V - 1), ("tile_end", tile - 1), ("tile_start", tile)):
        if 0 <= at < V:
            a = np.zeros(V, dtype=np.uint8)
            a[at] = 3
            fam["single_" + name] = a
    fam["foreign"] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 255], dtype=np.uint8), size=V)      # 4 reads as 3; 5 and 255 are nothing
    fam["mixed"] = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=V, p=[0.7, 0.1, 0.15, 0.05])
    runs = np.zeros(V, dtype=np.uint8)                       # 16-voxel runs: all of class 1, then none, then all of class 3, then none
    k = np.arange(V) // 16
    runs[k % 4 == 0] = 1
    runs[k % 4 == 2] = 3
    fam["runs16"] = runs
    lanes = np.zeros(V, dtype=np.uint8)                      # the same over the 64 voxels of a lane, with a lone class-2 voxel between
    k = np.arange(V) // 64
    lanes[k % 2 == 0] = 1
    lanes[(np.arange(V) % 128) == 100] = 2
    fam["lanes64"] = lanes
    return {k: v.reshape(shape) for k, v in fam.items()}


def ellipsoid_label(shape, seed=0):
    """three nested ellipsoids (classes 2 > 1 > 4, the enhancing core written as BraTS' label 4) in a background of 0, uint8"""
    rng = np.random.default_rng([seed, 77])
    c = [(0.35 + 0.3 * rng.random()) * s for s in shape]
    rad = (0.22 + 0.1 * rng.random()) * min(shape)
    g = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij", sparse=True)
    rr = np.sqrt(((g[0] - c[0]) / 1.0) ** 2 + ((g[1] - c[1]) / 1.2) ** 2 + ((g[2] - c[2]) / 0.9) ** 2)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[rr < rad] = 2
    lab[rr < 0.62 * rad] = 1
    lab[rr < 0.35 * rad] = 4
    return lab
