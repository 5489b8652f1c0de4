"""N3 -- BraTS-shaped data path.  The reference's `data/` package (ClsWiseBraTS128.BraDataSet128,
train_no_amp.py:19,156-165) is absent from its repository; what its training loop consumes is fixed by the call site
(train_no_amp.py:184-189): per sample ``x [4, 128,128,128] float32, target [128,128,128] int64 in {0..3},
edge [128,128,128] int64 in {0,1,2,4,5,6,7,8} (tools.py:174-218), missing_modal``.

Two map-style datasets produce exactly that tuple from 240 x 240 x 155 volumes with a random 128^3 crop:
  * ``SyntheticBraTS`` -- generator-defined volumes (no files; utils.synthetic), used by bench / tests / the harness default;
  * ``NpzBraTS``       -- one ``.npz`` per subject with ``image [4,H,W,D]`` (or ``[H,W,D,4]``) float and ``label [H,W,D]`` integer
                          (BraTS labels 0,1,2,4 -- 4 is mapped to 3 as the reference's loaders do).  nibabel is not available in
                          this image, so NIfTI conversion is left to the user (one ``np.savez`` per subject).
Edge codes are derived from the label with utils.synthetic.edge_codes (boundary of each sub-region, coded per E1/E2/E4).

``DeviceBraTS`` / ``prepare_batch`` produce the same tuple on the GPU (csrc/prep.hip: crop, optional flips and intensity scale / shift,
label remap and edge codes in one launch per eight samples; with a matrix in the parameters the crop is rotated and zoomed, trilinear for
the image and nearest for the label; with a control grid it is deformed elastically on top of that; with blur, noise or gamma in the
parameters csrc/intensity.hip then runs the intensity stage on the prepared crop; with a bias field, contrast or a low-resolution
zoom csrc/acquire.hip runs the acquisition stage before it), bit-equal to the CPU statement in this module, except gamma-mapped and
contrast-mapped channels, which are bounded (below: _intensity_stage_cpu, _acquisition_stage_cpu)."""
import glob
import math
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import synthetic as syn

FULL_SIZE = (240, 240, 155)


def random_crop_origin(full, crop, rng):
    """Uniform crop origin; volumes smaller than the crop along an axis are zero-padded at the far end (D = 155 -> 160 is the
    reference's input_D, train_no_amp.py:63)."""
    return tuple(int(rng.integers(0, max(f - c, 0) + 1)) for f, c in zip(full, crop))


def nonzero_boxes_host(a):
    """(box int32 [B, 6] = lo0, lo1, lo2, hi0, hi1, hi2 with hi exclusive, count int64 [B]) of a float32 array [B, 4, S0, S1, S2]:
    per sample the tightest box of the voxels with some channel whose bits & 0x7fffffff != 0 (+-0 is background; denormals,
    infinities and NaN are not) and their number; lo = S, hi = 0, count = 0 without one.  The numpy statement of cwf_nonzero_box."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    nz = ((a.view(np.uint32) & np.uint32(0x7fffffff)) != 0).any(axis=1)
    box = np.empty((a.shape[0], 6), dtype=np.int32)
    for b in range(a.shape[0]):
        for d in range(3):
            where = np.flatnonzero(nz[b].any(axis=tuple(k for k in range(3) if k != d)))
            box[b, d], box[b, 3 + d] = (where[0], where[-1] + 1) if where.size else (a.shape[2 + d], 0)
    return box, nz.reshape(a.shape[0], -1).sum(axis=1, dtype=np.int64)


def nonzero_box(image):
    """(lo, hi), two triples of Python ints with hi exclusive: the tightest box holding every nonzero voxel of one subject image
    float32 [4, S0, S1, S2] (nonzero_boxes_host's rule: the bits are tested), or None when the image is zero everywhere.  GPU
    tensors: HipBackend.nonzero_box and one copy of six integers to the host; CPU tensors: numpy.  The two are bit-equal."""
    if not (torch.is_tensor(image) and image.dtype == torch.float32 and image.dim() == 4 and image.shape[0] == 4 and image.numel() > 0):
        raise ValueError("nonzero_box: image must be a non-empty float32 [4, S0, S1, S2] tensor, got %s %s"
                         % (getattr(image, "dtype", type(image)), tuple(getattr(image, "shape", ()))))
    if image.is_cuda:
        from cwf import kernels
        box = kernels.backend().nonzero_box(image.contiguous()[None])[0].cpu().numpy()[0]
    else:
        box = nonzero_boxes_host(image.numpy()[None])[0][0]
    return _box_tuple(box)


def _box_tuple(box):
    """six integers lo | hi -> (lo, hi), None for the empty box (hi = 0)"""
    box = [int(v) for v in box]
    return None if box[3] == 0 else (tuple(box[:3]), tuple(box[3:]))


def box_crop_origin(full, crop, box, rng):
    """Crop origin inside the nonzero box = (lo, hi) of a volume of extent `full`: one rng.integers call per axis, as
    random_crop_origin makes.  Per axis, with a, b the box's lo and hi, c the crop and top = max(S - c, 0) (random_crop_origin's
    largest origin): the origin is uniform on [max(lo', 0), min(hi', top)] with [lo', hi'] = [a, b - c] when b - a >= c (the crop
    lies in the box) and [b - c, a] otherwise (the box lies in the crop).  The range is never empty, and every draw has
    |crop n box| = min(c, b - a) along the axis."""
    origin = []
    for s, c, a, b in zip(full, crop, box[0], box[1]):
        s, c, a, b = int(s), int(c), int(a), int(b)
        if not 0 <= a < b <= s:
            raise ValueError("box_crop_origin: the box (%r, %r) does not lie in a volume of extent %r" % (tuple(box[0]), tuple(box[1]), tuple(full)))
        lo, hi = (a, b - c) if b - a >= c else (b - c, a)
        origin.append(int(rng.integers(max(lo, 0), min(hi, max(s - c, 0)) + 1)))
    return tuple(origin)


def crop_pad(vol, origin, crop):
    """vol [..., H, W, D] -> [..., crop]; zero padding where the crop leaves the volume."""
    out = vol.new_zeros(vol.shape[:-3] + tuple(crop))
    sl_src, sl_dst = [], []
    for o, c, f in zip(origin, crop, vol.shape[-3:]):
        n = max(min(c, f - o), 0)
        sl_src.append(slice(o, o + n)); sl_dst.append(slice(0, n))
    out[(Ellipsis,) + tuple(sl_dst)] = vol[(Ellipsis,) + tuple(sl_src)]
    return out


class SyntheticBraTS(Dataset):
    """`n_subjects` deterministic synthetic subjects; each access draws a fresh random crop (seeded by (seed, epoch, index))."""

    def __init__(self, n_subjects=8, crop=(128, 128, 128), seed=1000, full_size=None):
        self.n, self.crop, self.seed, self.epoch = int(n_subjects), tuple(crop), int(seed), 0
        self.full = tuple(full_size) if full_size is not None else tuple(crop)   # default: generate the patch directly

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if self.full == self.crop:
            x, target, edge = syn.synthetic_sample(i + 7919 * self.epoch, self.crop, self.seed)
            return x, target, edge, torch.zeros(4, dtype=torch.bool)
        x, target, _ = syn.synthetic_sample(i, self.full, self.seed)
        rng = np.random.default_rng([self.seed, self.epoch, i])
        o = random_crop_origin(self.full, self.crop, rng)
        x, target = crop_pad(x, o, self.crop), crop_pad(target, o, self.crop)
        return x, target, syn.edge_codes(target), torch.zeros(4, dtype=torch.bool)


class NpzBraTS(Dataset):
    def __init__(self, root, list_file=None, crop=(128, 128, 128), seed=1000, train=True):
        if list_file is not None:
            with open(list_file) as f:
                names = [ln.strip() for ln in f if ln.strip()]
            self.paths = [os.path.join(root, n if n.endswith(".npz") else n + ".npz") for n in names]
        else:
            self.paths = sorted(glob.glob(os.path.join(root, "*.npz")))
        if not self.paths:
            raise FileNotFoundError("no .npz subjects under %s" % root)
        self.crop, self.seed, self.epoch, self.train = tuple(crop), int(seed), 0, bool(train)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        with np.load(self.paths[i], allow_pickle=False) as z:
            img, lab = z["image"], z["label"]
        img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32))
        if img.shape[-1] == 4 and img.shape[0] != 4:
            img = img.permute(3, 0, 1, 2).contiguous()
        lab = torch.from_numpy(np.ascontiguousarray(lab).astype(np.int64))
        lab[lab == 4] = 3
        if self.train:
            rng = np.random.default_rng([self.seed, self.epoch, i])
            o = random_crop_origin(tuple(lab.shape), self.crop, rng)
            img, lab = crop_pad(img, o, self.crop), crop_pad(lab, o, self.crop)
        return img, lab, syn.edge_codes(lab), torch.zeros(4, dtype=torch.bool)


# ------------------------------------------------------------------------------------------------------------------------------------
# Training batches prepared on the device.  The flip and intensity augmentations are this project's definitions (the TransBTS-family
# loaders the reference descends from flip each axis and shift intensities per channel; the reference's own `data/` package is absent),
# so they are opt-in and off by default.
ELASTIC_GRID_MIN, ELASTIC_GRID_MAX = 4, 8     # control points per axis of AugParams.disp
_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class AugParams:
    """Per-sample batch parameters: crop origin (3 ints), flips of the three crop axes, the per-channel intensity scale / shift
    (float32 [4] each; None = intensity off), matrix: the linear part M[d][j] of the output -> source map about the crop centre
    (nine float32 values, row-major; None = no resampling, the plain crop), and disp: the control grid of the elastic deformation,
    float32 [3, G0, G1, G2] with 4 <= G_d <= 8, displacements in voxels of the crop-local source coordinate (a read-only array; None =
    no deformation.  Non-finite control values are allowed: the voxels they reach read nothing).  The intensity stage on the prepared
    crop (_intensity_stage_cpu), per channel: blur, the Gaussian's sigma in voxels (float32 [4], 0 = off; None = all off); noise, the
    sigma of the additive noise (float32 [4], 0 = off) with noise_key, an int in [0, 2^63), the key of its counter-based stream;
    gamma, the exponent (float32 [4], 0 = off).  The acquisition stage, which runs before it (_acquisition_stage_cpu), per channel:
    bias, the control multipliers of the bias field, float32 [4, G0, G1, G2] with 4 <= G_d <= 8 and finite values > 0 (a read-only
    array; None = off), with bias_mask, four bools, the channels it applies to; contrast, the factor (float32 [4], 0 = off); lowres,
    the zoom of the coarse lattice in [0.5, 1) (float32 [4], 0 = off)."""
    __slots__ = ("origin", "flip", "scale", "shift", "matrix", "blur", "noise", "noise_key", "gamma", "bias_mask", "contrast", "lowres",
                 "disp", "bias")
    _ARRAYS = ("disp", "bias")            # compared bit for bit

    def __init__(self, origin, flip=(False, False, False), scale=None, shift=None, matrix=None, disp=None, *, blur=None, noise=None,
                 noise_key=None, gamma=None, bias=None, bias_mask=None, contrast=None, lowres=None):
        self.origin = tuple(int(o) for o in origin)
        self.flip = tuple(bool(f) for f in flip)
        if (scale is None) != (shift is None):
            raise ValueError("AugParams: scale and shift go together")
        self.scale = None if scale is None else tuple(float(v) for v in np.asarray(scale, dtype=np.float32))
        self.shift = None if shift is None else tuple(float(v) for v in np.asarray(shift, dtype=np.float32))
        if len(self.origin) != 3 or len(self.flip) != 3 or (self.scale is not None and (len(self.scale) != 4 or len(self.shift) != 4)):
            raise ValueError("AugParams: origin and flip take 3 values, scale and shift 4")
        self.matrix = None if matrix is None else tuple(float(v) for v in np.asarray(matrix, dtype=np.float32).reshape(-1))
        if self.matrix is not None and len(self.matrix) != 9:
            raise ValueError("AugParams: matrix takes 9 values")
        if disp is not None:
            disp = np.array(disp, dtype=np.float32, order="C")
            if disp.ndim != 4 or disp.shape[0] != 3 or not all(ELASTIC_GRID_MIN <= g <= ELASTIC_GRID_MAX for g in disp.shape[1:]):
                raise ValueError("AugParams: disp takes a [3, G0, G1, G2] grid with %d <= G_d <= %d, got shape %r"
                                 % (ELASTIC_GRID_MIN, ELASTIC_GRID_MAX, tuple(disp.shape)))
            disp.setflags(write=False)
        self.disp = disp
        for name, val in (("blur", blur), ("noise", noise), ("gamma", gamma)):
            if val is not None:
                val = tuple(float(v) for v in np.asarray(val, dtype=np.float32).reshape(-1))
                if len(val) != 4 or not all(np.isfinite(v) and v >= 0.0 for v in val):
                    raise ValueError("AugParams: %s takes 4 finite values >= 0 (0 = off), got %r" % (name, val))
            setattr(self, name, val)
        if noise_key is not None and not 0 <= int(noise_key) < 2 ** 63:
            raise ValueError("AugParams: noise_key must lie in [0, 2^63), got %r" % (noise_key,))
        self.noise_key = 0 if noise_key is None else int(noise_key)
        if bias is not None:
            bias = np.array(bias, dtype=np.float32, order="C")
            if bias.ndim != 4 or bias.shape[0] != 4 or not all(ELASTIC_GRID_MIN <= g <= ELASTIC_GRID_MAX for g in bias.shape[1:]):
                raise ValueError("AugParams: bias takes a [4, G0, G1, G2] grid with %d <= G_d <= %d, got shape %r"
                                 % (ELASTIC_GRID_MIN, ELASTIC_GRID_MAX, tuple(bias.shape)))
            if not bool(np.all(np.isfinite(bias) & (bias > 0))):
                raise ValueError("AugParams: bias takes finite control multipliers > 0")
            if bias_mask is None:
                raise ValueError("AugParams: bias comes with bias_mask, the four channels it applies to")
            bias.setflags(write=False)
        self.bias = bias
        mask = (False,) * 4 if bias_mask is None else tuple(bool(v) for v in bias_mask)
        if len(mask) != 4 or (bias is None and any(mask)):
            raise ValueError("AugParams: bias_mask takes 4 bools, and needs a bias where one is set, got %r" % (bias_mask,))
        self.bias_mask = mask
        for name, val, lo, hi in (("contrast", contrast, 0.0, np.inf), ("lowres", lowres, 0.5, 1.0)):
            if val is not None:
                val = tuple(float(v) for v in np.asarray(val, dtype=np.float32).reshape(-1))
                if len(val) != 4 or not all(v == 0.0 or (np.isfinite(v) and lo <= v < hi and v > 0.0) for v in val):
                    raise ValueError("AugParams: %s takes 4 values, each 0 (off) or %s, got %r"
                                     % (name, "finite and > 0" if name == "contrast" else "in [0.5, 1)", val))
            setattr(self, name, val)

    def at_origin(self, origin):
        return AugParams(origin, self.flip, self.scale, self.shift, self.matrix, self.disp, blur=self.blur, noise=self.noise,
                         noise_key=self.noise_key, gamma=self.gamma, bias=self.bias, bias_mask=self.bias_mask if self.bias is not None
                         else None, contrast=self.contrast, lowres=self.lowres)

    def intensity_stage(self):
        """True when blur, noise or gamma is on for some channel"""
        return any(v is not None and any(c > 0.0 for c in v) for v in (self.blur, self.noise, self.gamma))

    def acquisition_stage(self):
        """True when the bias field, contrast or the low-resolution simulation is on for some channel"""
        return any(self.bias_mask) or any(v is not None and any(c > 0.0 for c in v) for v in (self.contrast, self.lowres))

    def source_box(self, crop):
        """Integer bounds ((lo_0, hi_0), ...) relative to the origin, hi exclusive, that contain every source index the crop reads
        (both trilinear taps and the nearest label): the float64 range of q_d over the crop, widened by one voxel.  With a control
        grid axis d is widened further by ceil(max |disp[d]|) + 1 on both sides: the spline weights are non-negative and sum to 1
        within rounding, so |D_d| <= max |disp[d]| up to a few ulps (over the finite control values: a voxel that a non-finite one
        reaches reads nothing, and neither does one moved by 2^30 voxels or more)."""
        c = [(int(n) - 1) / 2.0 for n in crop]
        if self.matrix is None and self.disp is None:
            return tuple((0, int(n)) for n in crop)
        m = np.asarray(self.matrix if self.matrix is not None else _IDENTITY, dtype=np.float64).reshape(3, 3)
        box = []
        for d in range(3):
            r = sum(abs(m[d, j]) * c[j] for j in range(3))
            w = 0
            if self.disp is not None:
                a = np.abs(self.disp[d].astype(np.float64))
                a = a[np.isfinite(a)]
                w = int(min(np.ceil(a.max()) if a.size else 0.0, 2.0 ** 31)) + 1
            box.append((int(np.floor(c[d] - r)) - 1 - w, int(np.floor(c[d] + r)) + 3 + w))
        return tuple(box)

    def __eq__(self, other):
        if not isinstance(other, AugParams):
            return False
        if not all(getattr(self, k) == getattr(other, k) for k in self.__slots__ if k not in self._ARRAYS):
            return False
        for k in self._ARRAYS:
            a, b = getattr(self, k), getattr(other, k)
            if a is None or b is None:
                if a is not b:
                    return False
            elif a.shape != b.shape or a.tobytes() != b.tobytes():                                   # bit for bit (NaN included)
                return False
        return True

    def __repr__(self):
        head = "AugParams(origin=%r, flip=%r, scale=%r, shift=%r" % (self.origin, self.flip, self.scale, self.shift)
        head += "" if self.matrix is None else ", matrix=%r" % (self.matrix,)
        head += "" if self.blur is None else ", blur=%r" % (self.blur,)
        head += "" if self.noise is None else ", noise=%r, noise_key=%r" % (self.noise, self.noise_key)
        head += "" if self.gamma is None else ", gamma=%r" % (self.gamma,)
        if self.disp is not None:
            head += ", disp=float32%r max |.| %r" % (list(self.disp.shape), float(np.max(np.abs(self.disp))))
        if self.bias is not None:
            head += ", bias=float32%r in [%r, %r], bias_mask=%r" % (list(self.bias.shape), float(self.bias.min()),
                                                                    float(self.bias.max()), self.bias_mask)
        head += "" if self.contrast is None else ", contrast=%r" % (self.contrast,)
        head += "" if self.lowres is None else ", lowres=%r" % (self.lowres,)
        return head + ")"


def rotation_zoom_matrix(angles_deg, zoom=1.0):
    """float32 [9] (row-major) of Rz(gamma) . Ry(beta) . Rx(alpha) / zoom for angles (alpha, beta, gamma) in degrees about the crop's
    axes 0, 1, 2, computed in float64: the output -> source map of a patch rotated by the angles and magnified by `zoom`."""
    al, be, ga = (np.deg2rad(float(v)) for v in angles_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(al), -np.sin(al)], [0, np.sin(al), np.cos(al)]], dtype=np.float64)
    ry = np.array([[np.cos(be), 0, np.sin(be)], [0, 1, 0], [-np.sin(be), 0, np.cos(be)]], dtype=np.float64)
    rz = np.array([[np.cos(ga), -np.sin(ga), 0], [np.sin(ga), np.cos(ga), 0], [0, 0, 1]], dtype=np.float64)
    return ((rz @ ry @ rx) / float(zoom)).astype(np.float32).reshape(9)


FOREGROUND_CLASSES = (0b0010, 0b0100, 0b1000)    # the default regions of class_locations: classes 1, 2 and 3, each on its own
LOCATIONS_MAX_REGIONS, LOCATIONS_MAX_SAMPLES = 8, 65536


def _check_regions(posmasks, samples):
    masks, K = tuple(int(m) for m in posmasks), int(samples)
    if not 1 <= len(masks) <= LOCATIONS_MAX_REGIONS:
        raise ValueError("class_locations: takes 1..%d regions, got %d" % (LOCATIONS_MAX_REGIONS, len(masks)))
    if any(m < 0 or m > 0b1111 for m in masks):
        raise ValueError("class_locations: a region is a bitmask over classes 0..3, got %r" % (tuple(posmasks),))
    if not 1 <= K <= LOCATIONS_MAX_SAMPLES:
        raise ValueError("class_locations: the table length must lie in 1..%d, got %r" % (LOCATIONS_MAX_SAMPLES, samples))
    return masks, K


def class_locations(label, posmasks=FOREGROUND_CLASSES, samples=4096):
    """(counts int64 [R], table int32 [R, K]) of one subject's label uint8 [S0, S1, S2] (values 0..4 are classes, 4 read as 3; any
    other value belongs to no region), K = samples, on the label's device.  Region r is the class bitmask posmasks[r] over classes
    0..3 (1 <= R <= 8; regions may overlap).  counts[r] = n_r, its voxels; with m_r = min(n_r, K), table[r][j] for j < m_r is the
    C-order linear index of the region voxel of rank floor(j * n_r / m_r), ranks counted in increasing linear index, and -1 for
    j >= m_r: every voxel of the region when n_r <= K, an evenly ranked sample otherwise.  Exact integers throughout.
    GPU tensors: HipBackend.class_locations (bit-equal); CPU tensors: numpy."""
    masks, K = _check_regions(posmasks, samples)
    if label.dtype != torch.uint8 or not 1 <= label.numel() <= 2 ** 31 - 1:
        raise ValueError("class_locations: label must be a uint8 tensor of 1..2^31 - 1 voxels")
    if label.is_cuda:
        from cwf import kernels
        return kernels.backend().class_locations(label.contiguous(), masks, K)
    a = label.contiguous().numpy().reshape(-1)
    counts, table = np.zeros(len(masks), dtype=np.int64), np.full((len(masks), K), -1, dtype=np.int32)
    for r, mk in enumerate(masks):
        member = np.zeros(256, dtype=bool)
        member[:5] = [bool((mk >> c) & 1) for c in (0, 1, 2, 3, 3)]
        where = np.flatnonzero(member[a])
        n = int(where.size)
        m = min(n, K)
        counts[r] = n
        if m:
            table[r, :m] = where[(np.arange(m, dtype=np.int64) * n) // m]
    return torch.from_numpy(counts), torch.from_numpy(table)


def foreground_origin(seed, epoch, index, full, crop, counts, table, oversample):
    """The foreground draw of sample `index` in `epoch`, from a stream of its own, default_rng([seed, epoch, index, 1]) (no field of
    draw_params depends on it): u = random(); the crop is a foreground crop iff u < oversample and some region is non-empty.  Then
    r = the integers(0, #non-empty)-th non-empty region in region order, j = integers(0, min(counts[r], K)), v = the voxel whose
    linear index is table[r][j], and origin_d = clamp(v_d - crop_d // 2, 0, max(S_d - crop_d, 0)): inside random_crop_origin's range,
    with v inside [origin, origin + crop) whichever way the clamp acts and when S_d < crop_d.  Returns (origin, r, v), or
    (None, None, None) when the crop is not a foreground crop.  counts [R], table [R, K]: class_locations' result on the host."""
    counts, table = np.asarray(counts), np.asarray(table)
    rng = np.random.default_rng([int(seed), int(epoch), int(index), 1])
    u = rng.random()
    regions = [r for r in range(counts.shape[0]) if int(counts[r]) > 0]
    if not (u < float(oversample) and regions):
        return None, None, None
    r = regions[int(rng.integers(0, len(regions)))]
    j = int(rng.integers(0, min(int(counts[r]), table.shape[1])))
    v = tuple(int(c) for c in np.unravel_index(int(table[r][j]), tuple(int(s) for s in full)))
    origin = tuple(min(max(vd - c // 2, 0), max(s - c, 0)) for vd, c, s in zip(v, crop, full))
    return origin, r, v


def draw_params(seed, epoch, index, full, crop, flip=False, intensity=0.0, rotate=0.0, scale=0.0, elastic=0.0, elastic_grid=7,
                blur=0.0, noise=0.0, gamma=0.0, bias=0.0, bias_grid=4, contrast=0.0, lowres=0.0, oversample=0.0, foreground=None, box=None):
    """Parameters of sample `index` in `epoch`: a pure function of the arguments, drawn from default_rng([seed, epoch, index]).  The
    origin is drawn first, by random_crop_origin's calls, so with augmentation off it is the origin NpzBraTS / SyntheticBraTS pick.
    flip: three uniforms, each < 0.5 flipping that axis; intensity f > 0: scale ~ U(1-f, 1+f)[4], then shift ~ U(-f, f)[4] (float32).
    Drawn after all of those, so that they do not depend on it: rotate r > 0: three Euler angles ~ U(-r, r) degrees; scale f > 0: an
    isotropic zoom ~ U(1-f, 1+f); matrix = rotation_zoom_matrix(angles, zoom), None with both off.  Last of all, elastic e > 0: the
    control grid disp ~ U(-e, e) voxels, float32 [3, g, g, g] with g = elastic_grid; None with e = 0.  After everything above, so that
    no earlier field depends on them, the intensity stage, each transform switching a channel on where its u < 0.5 and making all its
    draws whatever the outcome: blur s (0, or 0.5 <= s <= 1.5): u = random(4), sigma ~ U(0.5, s)[4]; noise n > 0: u = random(4),
    sigma ~ U(0, n)[4], noise_key = integers(0, 2^63); gamma g (0 < g < 1): u = random(4), exponent ~ U(1-g, 1+g)[4].  A channel that
    is off has the value 0; a transform that is off is None.  Last, in the same manner, the acquisition stage: bias b (0 < b <= 1):
    u = random(4), a ~ U(-b, b)[4, g, g, g] with g = bias_grid, the control multipliers float32(exp(a)) (float64 exp: the field is
    positive without an exponential on the device), bias_mask = u < 0.5; contrast k (0 < k < 1): u = random(4), factor ~ U(1-k, 1+k)[4];
    lowres z (0.5 <= z < 1): u = random(4), zoom ~ U(z, 1)[4] (a zoom that float32 rounds to 1 becomes the float32 below 1).
    oversample p in [0, 1] with foreground = (counts, table), the subject's class_locations on the host: the uniform origin is drawn
    as ever and then replaced by foreground_origin's when that returns one (a stream of its own: nothing else moves).  With p = 0
    nothing new is called.
    box = (lo, hi), the subject's nonzero_box: the origin's three draws, still the first of the stream, are box_crop_origin's instead
    of random_crop_origin's, so the crop lies in the box or the box in the crop.  The ranges differ from the uniform ones, and a
    bounded draw may take a different number of words from the generator, so every later field may differ from a box-less call's.
    A foreground origin replaces this one as it replaces the uniform one.  With box = None nothing moves, bit for bit."""
    p = float(oversample)
    if not 0.0 <= p <= 1.0:
        raise ValueError("draw_params: oversample takes a probability in [0, 1], got %r" % (oversample,))
    if p > 0.0 and foreground is None:
        raise ValueError("draw_params: oversample > 0 needs foreground = (counts, table), the subject's class_locations")
    rng = np.random.default_rng([int(seed), int(epoch), int(index)])
    origin = random_crop_origin(tuple(full), tuple(crop), rng) if box is None else box_crop_origin(tuple(full), tuple(crop), box, rng)
    if p > 0.0:
        fg = foreground_origin(seed, epoch, index, full, crop, foreground[0], foreground[1], p)[0]
        origin = origin if fg is None else fg
    r, z = float(rotate), float(scale)
    fl = tuple(bool(u < 0.5) for u in rng.random(3)) if flip else (False, False, False)
    scale = shift = None
    f = float(intensity)
    if f > 0.0:
        scale = rng.uniform(1.0 - f, 1.0 + f, 4).astype(np.float32)
        shift = rng.uniform(-f, f, 4).astype(np.float32)
    matrix = None
    if r > 0.0 or z > 0.0:
        angles = rng.uniform(-r, r, 3) if r > 0.0 else np.zeros(3)
        zoom = float(rng.uniform(1.0 - z, 1.0 + z)) if z > 0.0 else 1.0
        matrix = rotation_zoom_matrix(angles, zoom)
    disp = None
    e, g = float(elastic), int(elastic_grid)
    if e > 0.0:
        disp = rng.uniform(-e, e, (3, g, g, g)).astype(np.float32)
    bl = ns = gm = key = None
    s, n, g = float(blur), float(noise), float(gamma)
    if s != 0.0 and not 0.5 <= s <= 1.5:
        raise ValueError("draw_params: blur takes 0 or a largest sigma in [0.5, 1.5], got %r" % (blur,))
    if n < 0.0 or not np.isfinite(n):
        raise ValueError("draw_params: noise takes a finite sigma >= 0, got %r" % (noise,))
    if not 0.0 <= g < 1.0:
        raise ValueError("draw_params: gamma takes a half-width in [0, 1), got %r" % (gamma,))
    if s > 0.0:
        u, sig = rng.random(4), rng.uniform(0.5, s, 4)
        bl = np.where(u < 0.5, sig, 0.0).astype(np.float32)
    if n > 0.0:
        u, sg, key = rng.random(4), rng.uniform(0.0, n, 4), int(rng.integers(0, 2 ** 63))
        ns = np.where(u < 0.5, sg, 0.0).astype(np.float32)
    if g > 0.0:
        u, ex = rng.random(4), rng.uniform(1.0 - g, 1.0 + g, 4)
        gm = np.where(u < 0.5, ex, 0.0).astype(np.float32)
    b, bg, k, zmin = float(bias), int(bias_grid), float(contrast), float(lowres)
    if not 0.0 <= b <= 1.0:
        raise ValueError("draw_params: bias takes a half-width of the log multiplier in [0, 1], got %r" % (bias,))
    if b > 0.0 and not ELASTIC_GRID_MIN <= bg <= ELASTIC_GRID_MAX:
        raise ValueError("draw_params: bias_grid takes %d..%d control points per axis, got %r" % (ELASTIC_GRID_MIN, ELASTIC_GRID_MAX, bias_grid))
    if not 0.0 <= k < 1.0:
        raise ValueError("draw_params: contrast takes a half-width in [0, 1), got %r" % (contrast,))
    if zmin != 0.0 and not 0.5 <= zmin < 1.0:
        raise ValueError("draw_params: lowres takes 0 or a smallest zoom in [0.5, 1), got %r" % (lowres,))
    bf = bm = ct = lr = None
    if b > 0.0:
        u, a = rng.random(4), rng.uniform(-b, b, (4, bg, bg, bg))
        bf, bm = np.exp(a).astype(np.float32), tuple(bool(v) for v in u < 0.5)
    if k > 0.0:
        u, fc = rng.random(4), rng.uniform(1.0 - k, 1.0 + k, 4)
        ct = np.where(u < 0.5, fc, 0.0).astype(np.float32)
    if zmin > 0.0:
        u, zm = rng.random(4), rng.uniform(zmin, 1.0, 4)
        zm = np.minimum(zm.astype(np.float32), np.nextafter(np.float32(1.0), np.float32(0.0)))
        lr = np.where(u < 0.5, zm, np.float32(0.0)).astype(np.float32)
    return AugParams(origin, fl, scale, shift, matrix, disp, blur=bl, noise=ns, noise_key=key, gamma=gm, bias=bf, bias_mask=bm,
                     contrast=ct, lowres=lr)


_Q_MAX = np.float32(2.0 ** 30)      # |q| at and beyond it (and NaN): the voxel lies outside every volume


def _affine_coords(p, crop):
    """q [3, *crop] float32 of the affine part of the statement in _resample_cpu (the identity matrix when p has none), and
    ok [*crop]: every |q_d| < 2^30"""
    q, ok = [], np.ones(tuple(crop), dtype=bool)
    c = [np.float32(n - 1) * np.float32(0.5) for n in crop]
    u = []
    for d in range(3):
        pd = np.arange(crop[d], dtype=np.int64)
        if p.flip[d]:
            pd = crop[d] - 1 - pd
        u.append((pd.astype(np.float32) - c[d]).reshape([-1 if k == d else 1 for k in range(3)]))
    m = np.asarray(p.matrix if p.matrix is not None else _IDENTITY, dtype=np.float32).reshape(3, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(3):
            qd = ((m[d, 0] * u[0] + m[d, 1] * u[1]) + m[d, 2] * u[2]) + c[d]
            ok &= np.abs(qd) < _Q_MAX               # (False for NaN)
            q.append(qd)
    return q, ok


def _spline_axis(n, flip, g):
    """(w float32 [n, 4], index int64 [n, 4]) of the cubic B-spline along one crop axis of n voxels and g control points"""
    f32 = np.float32
    pd = np.arange(n, dtype=np.int64)
    if flip:
        pd = n - 1 - pd
    k = f32(g - 3) / f32(n - 1) if n > 1 else f32(0.0)
    gd = pd.astype(f32) * k + f32(1.0)
    fl = np.floor(gd)
    t = gd - fl
    s = f32(1.0) - t
    h = f32(1.0 / 6.0)
    w = np.stack([((s * s) * s) * h,
                  ((((f32(3.0) * t - f32(6.0)) * t) * t) + f32(4.0)) * h,
                  ((((f32(-3.0) * t + f32(3.0)) * t + f32(3.0)) * t) + f32(1.0)) * h,
                  ((t * t) * t) * h], axis=1).astype(f32)
    idx = np.clip(fl.astype(np.int64)[:, None] - 1 + np.arange(4, dtype=np.int64)[None, :], 0, g - 1)
    return w, idx


def _elastic_disp(p, crop):
    """D [3][*crop] float32 of the statement in _resample_cpu.  The nested sums are taken axis by axis -- axis 2 over the whole control
    grid, then axis 1, then axis 0 -- which forms, for every voxel, the same products and sums in the same order."""
    w, idx = zip(*(_spline_axis(crop[d], p.flip[d], p.disp.shape[1 + d]) for d in range(3)))

    def sum4(term):
        return ((term(0) + term(1)) + term(2)) + term(3)

    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(3):
            a = sum4(lambda j: w[2][:, j] * p.disp[c][:, :, idx[2][:, j]])                               # [G0, G1, C2]
            b = sum4(lambda j: w[1][:, j, None] * a[:, idx[1][:, j], :])                                 # [G0, C1, C2]
            out.append(sum4(lambda j: w[0][:, j, None, None] * b[idx[0][:, j], :, :]).astype(np.float32))   # [C0, C1, C2]
    return out


def _source_coords(p, crop):
    """q [3][*crop] float32 of the statement in _resample_cpu, and ok [*crop]: every |q_d| < 2^30"""
    q, ok = _affine_coords(p, crop)
    if p.disp is None:
        return q, ok
    D = _elastic_disp(p, crop)
    ok = np.ones(tuple(crop), dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        q = [np.broadcast_to(q[d], tuple(crop)) + D[d] for d in range(3)]
        for d in range(3):
            ok &= np.abs(q[d]) < _Q_MAX
    return q, ok


def _resample_cpu(img, lab, p, crop):
    """The resampled crop, numpy float32 with one rounding per operation.  With c_d = (C_d - 1) / 2, o the origin, p the output voxel:
        p'_d = flip_d ? C_d - 1 - p_d : p_d                       (resample, then torch.flip of the result)
        u_d  = float(p'_d) - c_d
        q_d  = ((M[d][0]*u_0 + M[d][1]*u_1) + M[d][2]*u_2) + c_d   crop-local source coordinate (M = identity without a matrix)
      with a control grid disp [3, G0, G1, G2] (a uniform cubic B-spline of p', displacements in voxels of q), along each axis d
        k_d  = float32(G_d - 3) / float32(C_d - 1)                 (correctly rounded; 0 when C_d == 1)
        g_d  = p'_d * k_d + 1;  i_d = floor(g_d);  t = g_d - i_d;  s = 1 - t;  h = float32(1/6)
        w0 = ((s*s)*s)*h   w1 = ((((3*t - 6)*t)*t) + 4)*h   w2 = ((((-3*t + 3)*t + 3)*t) + 1)*h   w3 = ((t*t)*t)*h
        control index for j = 0..3: clamp(i_d - 1 + j, 0, G_d - 1)  (only i_d + 2 == G_d is ever clamped, where w3 is 0 or one
                                                                    rounding away from it)
        D_c  = sum_j0 w[0][j0] * (sum_j1 w[1][j1] * (sum_j2 w[2][j2] * disp[c][..][..][..])), every 4-term sum as ((a + b) + c) + d
        q_c  = q_c + D_c                                           (no grid: nothing is added)
        image: i_d = floor(q_d), f_d = q_d - i_d, the eight taps at source index o_d + i_d + {0, 1}, 0.0 where an index leaves
               [0, S_d); lerp(a, b, f) = a + f*(b - a) along axis 2, then axis 1, then axis 0
        label: label[o + floor(q + 0.5)], 0 outside the volume
    A voxel with some final |q_d| >= 2^30 or NaN (a NaN or huge control value gives one) reads nothing: image 0.0, label 0.  The origin enters only as an integer added to the
    indices, so the result does not change when the source is cut to a box and the origin moved with it."""
    crop = tuple(int(c) for c in crop)
    a, l = img.numpy(), lab.numpy()
    S = l.shape
    q, ok = _source_coords(p, crop)
    idx, fr, nn = [], [], []
    for d in range(3):
        qd = np.where(ok, q[d], np.float32(0.0)).astype(np.float32)
        fl = np.floor(qd)
        fr.append(qd - fl)
        idx.append(fl.astype(np.int64) + p.origin[d])
        nn.append(np.floor(qd + np.float32(0.5)).astype(np.int64) + p.origin[d])

    def inside(i, d):
        return (i >= 0) & (i < S[d])

    x = np.empty((4,) + crop, dtype=np.float32)
    taps = {}
    for d0 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                i0, i1, i2 = idx[0] + d0, idx[1] + d1, idx[2] + d2
                m = ok & inside(i0, 0) & inside(i1, 1) & inside(i2, 2)
                taps[d0, d1, d2] = (m, np.clip(i0, 0, S[0] - 1), np.clip(i1, 0, S[1] - 1), np.clip(i2, 0, S[2] - 1))

    def lerp(lo, hi, f):
        return lo + f * (hi - lo)

    for c in range(4):
        v = {k: np.where(m, a[c][i0, i1, i2], np.float32(0.0)).astype(np.float32) for k, (m, i0, i1, i2) in taps.items()}
        r1 = {(d0, d1): lerp(v[d0, d1, 0], v[d0, d1, 1], fr[2]) for d0 in (0, 1) for d1 in (0, 1)}
        r0 = [lerp(r1[d0, 0], r1[d0, 1], fr[1]) for d0 in (0, 1)]
        x[c] = lerp(r0[0], r0[1], fr[0])
    m = ok & inside(nn[0], 0) & inside(nn[1], 1) & inside(nn[2], 2)
    t = np.where(m, l[np.clip(nn[0], 0, S[0] - 1), np.clip(nn[1], 0, S[1] - 1), np.clip(nn[2], 0, S[2] - 1)], 0).astype(np.int64)
    return torch.from_numpy(x), torch.from_numpy(t)


BLUR_RADIUS = 3                                 # the Gaussian is truncated here: seven taps
NOISE_DIV = np.sqrt((65536.0 ** 2 - 1.0) / 3.0)   # the standard deviation of the sum of four uniform 16-bit integers


def blur_taps64(sigma):
    """the seven taps before their rounding to float32, as Python floats (the per-batch path of HipBackend.prepare_batch takes them
    from here: a few microseconds per channel)"""
    sg = float(np.float32(sigma))
    e = [math.exp(-0.5 * ((j / sg) * (j / sg))) for j in range(-BLUR_RADIUS, BLUR_RADIUS + 1)]
    total = sum(e)
    return [v / total for v in e]


def blur_taps(sigma):
    """float32 [7]: w[j] = exp(-0.5 ((j - 3) / sigma)^2) / sum_j exp(...), in float64 from the float32 sigma"""
    return np.array(blur_taps64(sigma), dtype=np.float64).astype(np.float32)


def noise_amp64(sigma):
    return float(np.float32(sigma)) / NOISE_DIV


def noise_amp(sigma):
    """float32(sigma / D), D = sqrt((65536^2 - 1) / 3), in float64 from the float32 sigma"""
    return np.float32(noise_amp64(sigma))


def noise_ints(key, start, n):
    """int64 [n]: s of the statement in _intensity_stage_cpu for the counters key + start .. key + start + n - 1 (wrapping)"""
    with np.errstate(over="ignore"):
        ctr = np.arange(int(start), int(start) + int(n), dtype=np.uint64) + np.uint64(int(key))
    h = syn._splitmix64(ctr)
    m = np.uint64(0xFFFF)
    s = (h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))
    return s.astype(np.int64) - 131070


def _blur_axis_cpu(a, w, axis):
    n = a.shape[axis]
    pad = np.take(a, np.clip(np.arange(-BLUR_RADIUS, n + BLUR_RADIUS), 0, n - 1), axis=axis)
    tap = [w[j] * np.take(pad, np.arange(j, j + n), axis=axis) for j in range(2 * BLUR_RADIUS + 1)]
    y = tap[0] + tap[1]
    for j in range(2, 2 * BLUR_RADIUS + 1):
        y = y + tap[j]
    return y.astype(np.float32)


def _intensity_stage_cpu(x, p):
    """The intensity stage on the prepared crop x [4, C0, C1, C2] (numpy float32, changed in place), every operation a float32
    round-to-nearest one in the association written.  With V = C0*C1*C2 and v = (p0*C1 + p1)*C2 + p2, per channel c, in this order:
      blur (sigma_c > 0): taps w = blur_taps(sigma_c) (radius 3: this project's definition); along axis 2, then 1, then 0
          y[p] = (((((w0*a[p-3] + w1*a[p-2]) + w2*a[p-1]) + w3*a[p]) + w4*a[p+1]) + w5*a[p+2]) + w6*a[p+3]
        with indices clamped to [0, C_d - 1]: the border is the crop's own (replicate); zeros from padding outside the volume are data
      noise (sigma_c > 0): h = splitmix64(noise_key + uint64(c*V + v)), s = the sum of h's four 16-bit fields - 131070,
          x = x + float32(s) * amp_c, amp_c = noise_amp(sigma_c): a sum of four uniforms, bounded at +-3.46 sigma, not a true normal
      gamma (gamma_c > 0): mn, mx the NaN-ignoring minimum and maximum of the channel after the steps above, r = mx - mn; when r is
          finite and > 0: u = (x - mn) / r, x = pow(u, gamma_c) * r + mn with a float32 power
    A step that is off leaves the channel's bits alone.  The device differs from this only in the power: its powf is within a few
    ulps of the correctly rounded one, so a gamma-mapped channel is bounded, not bit-equal."""
    V = int(x[0].size)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for c in range(4):
            if p.blur is not None and p.blur[c] > 0.0:
                w = blur_taps(p.blur[c])
                a = x[c]
                for axis in (2, 1, 0):
                    a = _blur_axis_cpu(a, w, axis)
                x[c] = a
            if p.noise is not None and p.noise[c] > 0.0:
                s = noise_ints(p.noise_key, c * V, V).astype(np.float32).reshape(x[c].shape)
                x[c] = x[c] + s * noise_amp(p.noise[c])
            if p.gamma is not None and p.gamma[c] > 0.0:
                mn, mx = np.fmin.reduce(x[c], axis=None), np.fmax.reduce(x[c], axis=None)
                r = np.float32(mx - mn)
                if np.isfinite(r) and r > 0:
                    u = ((x[c] - mn) / r).astype(np.float32)
                    x[c] = np.power(u, np.float32(p.gamma[c])).astype(np.float32) * r + mn
    return x


def bias_field(grid, crop):
    """m [*crop] float32 of the statement in _acquisition_stage_cpu for one channel's control multipliers grid [G0, G1, G2]: the
    spline of _elastic_disp at the unflipped crop index, the nested sums taken axis by axis as there"""
    w, idx = zip(*(_spline_axis(crop[d], False, grid.shape[d]) for d in range(3)))

    def sum4(term):
        return ((term(0) + term(1)) + term(2)) + term(3)

    a = sum4(lambda j: w[2][:, j] * grid[:, :, idx[2][:, j]])                                    # [G0, G1, C2]
    b = sum4(lambda j: w[1][:, j, None] * a[:, idx[1][:, j], :])                                 # [G0, C1, C2]
    return sum4(lambda j: w[0][:, j, None, None] * b[idx[0][:, j], :, :]).astype(np.float32)     # [C0, C1, C2]


def lowres_lattice(crop, zoom):
    """(n_0, n_1, n_2): n_d = min(C_d, max(1, floor(float64(C_d) * zoom + 0.5))) for the float32 zoom"""
    z = float(np.float32(zoom))
    return tuple(min(int(c), max(1, int(math.floor(float(c) * z + 0.5)))) for c in crop)


def _lowres_axis(C, n):
    """(lo int64 [C], hi int64 [C], t float32 [C]): the crop indices of the two taps and the fraction, along one axis of C voxels
    interpolated back from n lattice points"""
    f32 = np.float32
    r = f32(n) / f32(C)
    u = (np.arange(C, dtype=np.int64).astype(f32) + f32(0.5)) * r - f32(0.5)
    u = np.minimum(np.maximum(u, f32(0.0)), f32(n - 1)).astype(f32)
    k = np.maximum(np.minimum(np.floor(u).astype(np.int64), n - 2), 0)
    t = (u - k.astype(f32)).astype(f32)
    k1 = np.minimum(k + 1, n - 1)
    return ((2 * k + 1) * C) // (2 * n), ((2 * k1 + 1) * C) // (2 * n), t


def _acquisition_stage_cpu(x, p):
    """The acquisition stage on the prepared crop x [4, C0, C1, C2] (numpy float32, changed in place), before _intensity_stage_cpu;
    every operation a float32 round-to-nearest one in the association written.  With V = C0*C1*C2 and p = (p0, p1, p2) the crop
    voxel, per channel c, in this order (all three are this project's definitions):
      bias field (bias_mask[c]): x = x * m(p), m(p) = sum_j0 w0[j0] * (sum_j1 w1[j1] * (sum_j2 w2[j2] * bias[c][i0+j0][i1+j1][i2+j2]))
          with the weights, clamped control indices and ((a + b) + c) + d sums of _resample_cpu's D_c at the unflipped crop index
          (bias_field).  The weights are non-negative and sum to 1 within rounding, so m lies between the smallest and the largest
          control multiplier up to a few ulps: smooth and positive.
      contrast (contrast[c] = f > 0): S = the float64 sum of the channel, mean = float32(S / V); mn, mx the NaN-ignoring minimum and
          maximum; when mean is finite: x = min(max(((x - mean) * f) + mean, mn), mx)
      low resolution (lowres[c] = z in [0.5, 1)): the lattice n = lowres_lattice(crop, z); lattice point k along axis d samples crop
          index s_d(k) = ((2k + 1) * C_d) // (2 * n_d); back to the crop, r_d = float32(n_d) / float32(C_d),
          u = (float32(p_d) + 0.5) * r_d - 0.5 clamped to [0, n_d - 1], k = min(floor(u), n_d - 2) (0 when n_d == 1), t = u - k, taps
          s_d(k) and s_d(min(k + 1, n_d - 1)); lerp(a, b, t) = a + t*(b - a) along axis 2, then 1, then 0, over the channel as the
          contrast step left it.  With n_d == C_d the taps are p_d and p_d + 1 and t = 0, except at p_d = C_d - 1 > 0, where they are
          p_d - 1 and p_d and t = 1: the step returns a + 0*(b - a) = a (finite values; -0.0 may become 0.0), and a + (b - a) on those
          last planes, which is b up to one rounding of b - a.
    A step that is off leaves the channel's bits alone.  The device differs from this only in S: its float64 sum is taken in another
    (fixed) order than numpy's, so a contrast-mapped channel is bit-equal where the sum is exact and bounded otherwise
    (tests/test_acquisition_prepare_gpu.py)."""
    crop = tuple(int(n) for n in x.shape[1:])
    V = int(x[0].size)
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for c in range(4):
            if p.bias_mask[c]:
                x[c] = x[c] * bias_field(p.bias[c], crop)
            if p.contrast is not None and p.contrast[c] > 0.0:
                mean = f32(x[c].astype(np.float64).sum() / V)
                mn, mx = np.fmin.reduce(x[c], axis=None), np.fmax.reduce(x[c], axis=None)
                if np.isfinite(mean):
                    x[c] = np.minimum(np.maximum(((x[c] - mean) * f32(p.contrast[c])) + mean, mn), mx)
            if p.lowres is not None and p.lowres[c] > 0.0:
                (l0, h0, t0), (l1, h1, t1), (l2, h2, t2) = (_lowres_axis(C, n) for C, n in zip(crop, lowres_lattice(crop, p.lowres[c])))
                a = x[c]

                def lerp(lo, hi, t):
                    return lo + t * (hi - lo)

                a = lerp(a[:, :, l2], a[:, :, h2], t2[None, None, :]).astype(f32)
                a = lerp(a[:, l1, :], a[:, h1, :], t1[None, :, None]).astype(f32)
                x[c] = lerp(a[l0], a[h0], t0[:, None, None]).astype(f32)
    return x


def _prepare_one_cpu(img, lab, p, crop):
    if p.matrix is not None or p.disp is not None:
        x, t = _resample_cpu(img, lab, p, crop)
    else:
        x = crop_pad(img, p.origin, crop)
        t = crop_pad(lab.to(torch.int64), p.origin, crop)
        dims = [d for d in range(3) if p.flip[d]]
        if dims:
            x = torch.flip(x, [d + 1 for d in dims])
            t = torch.flip(t, dims)
    if p.scale is not None:
        x = x * torch.tensor(p.scale, dtype=torch.float32).reshape(4, 1, 1, 1)
        x = x + torch.tensor(p.shift, dtype=torch.float32).reshape(4, 1, 1, 1)
    if p.acquisition_stage():
        x = torch.from_numpy(_acquisition_stage_cpu(np.array(x.numpy(), dtype=np.float32, order="C"), p))
    if p.intensity_stage():
        x = torch.from_numpy(_intensity_stage_cpu(np.array(x.numpy(), dtype=np.float32, order="C"), p))
    t[t == 4] = 3
    return x, t, syn.edge_codes(t)


def prepare_batch(images, labels, params, crop, out=None):
    """(x [B,4,*crop] float32, target [B,*crop] int64, edge [B,*crop] int64) from source volumes images[b] float32 [4,S0,S1,S2] and
    labels[b] uint8 [S0,S1,S2] (values 0..4): crop_pad at params[b].origin (with params[b].matrix or .disp: the resampled crop of
    _resample_cpu, any origin) -> torch.flip of the flipped crop axes -> x * scale then + shift in float32 -> label 4 -> 3 ->
    utils.synthetic.edge_codes; with params[b].bias / .contrast / .lowres the acquisition stage (_acquisition_stage_cpu) then acts
    on x (bit-equal on the GPU except contrast-mapped channels, whose mean comes from another summation order); with
    params[b].blur / .noise / .gamma the intensity stage (_intensity_stage_cpu) acts on x after it.  On GPU tensors this is one HIP launch per eight samples, plus the stage's when it is on
    (HipBackend.prepare_batch, bit-equal to the CPU statement except gamma-mapped channels); on CPU tensors it is the CPU statement itself.  out: (x, target, edge)
    to write into (sample stride free, samples contiguous)."""
    crop = tuple(int(c) for c in crop)
    if len(images) and images[0].is_cuda:
        from cwf import kernels
        return kernels.backend().prepare_batch(images, labels, params, crop, out=out)
    xs, ts, es = zip(*(_prepare_one_cpu(i, l, p, crop) for i, l, p in zip(images, labels, params)))
    x, t, e = torch.stack(xs), torch.stack(ts), torch.stack(es)
    if out is None:
        return x, t, e
    for dst, src in zip(out, (x, t, e)):
        dst.copy_(src)
    return tuple(out)


def normalize_nonzero(image):
    """In place: z-score each channel of image [4,H,W,D] float32 over the voxels whose four-channel sum ((x0 + x1) + x2) + x3 is > 0,
    float64 two-pass mean and population std; masked voxels become float32((x - mean) / std), the rest and channels with std 0 stay.
    GPU tensors: HipBackend.normalize_nonzero; CPU tensors: numpy float64."""
    if image.is_cuda:
        from cwf import kernels
        return kernels.backend().normalize_nonzero(image)
    a = image.numpy()
    s = ((a[0] + a[1]) + a[2]) + a[3]
    m = s > 0
    if m.any():
        for c in range(4):
            v = a[c][m].astype(np.float64)
            mean = v.sum() / v.size
            std = np.sqrt(((v - mean) ** 2).sum() / v.size)
            if std > 0:
                a[c][m] = ((v - mean) / std).astype(np.float32)
    return image


def _npz_paths(root, list_file=None):
    if list_file is not None:
        with open(list_file) as f:
            names = [ln.strip() for ln in f if ln.strip()]
        paths = [os.path.join(root, n if n.endswith(".npz") else n + ".npz") for n in names]
    else:
        paths = sorted(glob.glob(os.path.join(root, "*.npz")))
    if not paths:
        raise FileNotFoundError("no .npz subjects under %s" % root)
    return paths


def _npz_shapes(path):
    """(image shape, label shape) read from the .npy headers inside an .npz, without loading the arrays."""
    import zipfile
    out = {}
    with zipfile.ZipFile(path) as zf:
        for key in ("image", "label"):
            with zf.open(key + ".npy") as f:
                version = np.lib.format.read_magic(f)
                read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
                out[key] = read(f)[0]
    return out["image"], out["label"]


def _label_array(lab, name):
    """label -> uint8 [H,W,D] with values in {0,1,2,3,4} (a CPU tensor)"""
    lab = np.asarray(lab.numpy() if isinstance(lab, torch.Tensor) else lab)
    if lab.size and (lab.min() < 0 or lab.max() > 4 or np.any(lab != np.round(lab))):
        bad = sorted(set(np.unique(lab).tolist()) - {0, 1, 2, 3, 4})
        raise ValueError("%s: label values must lie in {0, 1, 2, 3, 4} (BraTS labels), found %s" % (name, bad[:8]))
    return torch.from_numpy(np.ascontiguousarray(lab.astype(np.uint8)))


def _subject_arrays(img, lab, name):
    """image -> float32 [4,H,W,D] (accepting [H,W,D,4]), label -> uint8 [H,W,D] with values in {0,1,2,3,4} (CPU tensors)."""
    img = torch.as_tensor(np.ascontiguousarray(img.numpy() if isinstance(img, torch.Tensor) else img, dtype=np.float32))
    if img.shape[-1] == 4 and img.shape[0] != 4:
        img = img.permute(3, 0, 1, 2)
    img = img.contiguous()
    lab = _label_array(lab, name)
    if img.dim() != 4 or img.shape[0] != 4 or tuple(img.shape[1:]) != tuple(lab.shape):
        raise ValueError("%s: image %s and label %s do not form one [4,H,W,D] / [H,W,D] subject" % (name, tuple(img.shape), tuple(lab.shape)))
    return img, lab


class NpzCropSource(Dataset):
    """Map-style dataset of the staged device path (DeviceBraTS(cache=False)), run in DataLoader workers: item i is the crop of subject
    i at draw_params' origin, before any flip or intensity -- (image float32 [4,*crop], label uint8 [*crop], index) -- from one
    np.load + crop_pad (no edge codes).  `subjects`: .npz paths, or in-memory (image, label) pairs.  With rotate / scale / elastic on, the
    item is instead the part of the volume the resampled crop reads (staged_box: shapes differ from item to item); flip and
    intensity are taken only because they move the matrix's place in draw_params' stream.  DeviceBraTS's blur / noise / gamma are not
    taken: draw_params draws them after the matrix and the grid, so they move nothing this class reads, and they act on the prepared
    crop only, so the item is the same with and without them; the same holds for its bias / contrast / lowres, drawn last of all.
    oversample > 0 with foreground, the per-subject list of host (counts, table) pairs of class_locations: the origin is draw_params'
    foreground-oversampled one, on the plain-crop path and the staged_box path alike.
    crop_nonzero: the origin is draw_params' box origin, inside the subject's nonzero box.  The box is taken from the raw image the
    item has just loaded, before normalize_nonzero, by the numpy statement (nonzero_boxes_host) and memoised per subject in `boxes`
    (index -> six integers lo | hi); the item then carries it as a fourth element, so that the process that prepares the batch
    learns it from a DataLoader worker without loading the subject itself.  A subject that is zero everywhere is drawn as if the
    option were off."""

    def __init__(self, subjects, crop, seed=1000, normalize=False, flip=False, intensity=0.0, rotate=0.0, scale=0.0, elastic=0.0,
                 elastic_grid=7, oversample=0.0, foreground=None, crop_nonzero=False):
        self.crop_nonzero, self.boxes = bool(crop_nonzero), {}
        self.oversample, self.foreground = float(oversample), foreground
        if not 0.0 <= self.oversample <= 1.0:
            raise ValueError("NpzCropSource: oversample takes a probability in [0, 1], got %r" % (oversample,))
        if self.oversample > 0.0 and (foreground is None or len(foreground) != len(subjects)):
            raise ValueError("NpzCropSource: oversample > 0 needs foreground, one (counts, table) pair per subject")
        self.subjects, self.crop, self.seed, self.normalize, self.epoch = list(subjects), tuple(crop), int(seed), bool(normalize), 0
        self.flip, self.intensity, self.rotate, self.scale = bool(flip), float(intensity), float(rotate), float(scale)
        self.elastic, self.elastic_grid = float(elastic), int(elastic_grid)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.subjects)

    def _foreground(self, i):
        """draw_params' two keywords for subject i"""
        if self.oversample > 0.0:
            return {"oversample": self.oversample, "foreground": self.foreground[i]}
        return {}

    def box(self, i):
        """subject i's nonzero box as six integers lo | hi (hi = 0: empty); loads the subject when no one has yet"""
        if i not in self.boxes:
            self.load(i)
        return self.boxes[i]

    def _origin_keywords(self, i):
        """draw_params' keywords that move the origin of subject i: _foreground's and, with crop_nonzero, the box"""
        kw = self._foreground(i)
        box = _box_tuple(self.box(i)) if self.crop_nonzero else None
        return kw if box is None else dict(kw, box=box)

    def load_label(self, i):
        """subject i's label alone, uint8 (only the label array of an .npz is read)"""
        s = self.subjects[i]
        if isinstance(s, str):
            with np.load(s, allow_pickle=False) as z:
                return _label_array(z["label"], s)
        lab = s[1]
        return lab if isinstance(lab, torch.Tensor) and lab.dtype == torch.uint8 else _label_array(lab, "subject %d" % i)

    def load(self, i):
        s = self.subjects[i]
        if isinstance(s, str):
            with np.load(s, allow_pickle=False) as z:
                img, lab = _subject_arrays(z["image"], z["label"], s)
        else:
            img, lab = s
            if not (isinstance(img, torch.Tensor) and img.dtype == torch.float32 and img.dim() == 4 and img.shape[0] == 4
                    and lab.dtype == torch.uint8):
                img, lab = _subject_arrays(img, lab, "subject %d" % i)
            elif self.normalize:
                img = img.clone()
        if self.crop_nonzero and i not in self.boxes:
            self.boxes[i] = tuple(int(v) for v in nonzero_boxes_host(img.numpy()[None])[0][0])
        if self.normalize:
            normalize_nonzero(img)
        return img, lab

    def __getitem__(self, i):
        img, lab = self.load(i)
        if self.rotate > 0.0 or self.scale > 0.0 or self.elastic > 0.0:
            p = draw_params(self.seed, self.epoch, i, tuple(lab.shape), self.crop, self.flip, self.intensity, self.rotate, self.scale,
                            self.elastic, self.elastic_grid, **self._origin_keywords(i))
            (a0, b0), (a1, b1), (a2, b2) = staged_box(p, tuple(lab.shape), self.crop)
            item = img[:, a0:b0, a1:b1, a2:b2].contiguous(), lab[a0:b0, a1:b1, a2:b2].contiguous(), i
        else:
            o = draw_params(self.seed, self.epoch, i, tuple(lab.shape), self.crop, **self._origin_keywords(i)).origin
            item = crop_pad(img, o, self.crop), crop_pad(lab, o, self.crop), i
        return item + (self.boxes[i],) if self.crop_nonzero else item


def staged_box(p, extents, crop):
    """((lo_0, hi_0), ...) in volume indices: origin + p.source_box(crop) clipped to the volume, never empty.  Every index the
    resampled crop reads inside the volume lies in it, so preparing from volume[box] at origin - lo gives the same batch."""
    box = []
    for o, (lo, hi), s in zip(p.origin, p.source_box(crop), extents):
        lo = min(max(o + lo, 0), s - 1)
        box.append((lo, min(max(o + hi, lo + 1), s)))
    return tuple(box)


def _collate_crops(items, stack=True):
    imgs, labs, idx, *boxes = zip(*items)
    boxes = tuple(list(b) for b in boxes)   # crop_nonzero: the subjects' nonzero boxes as a fourth element
    if not stack:                       # source boxes of resampled crops: one shape per item
        return (list(imgs), list(labs), list(idx)) + boxes
    return (torch.stack(imgs), torch.stack(labs), list(idx)) + boxes


def _collate_boxes(items):
    return _collate_crops(items, stack=False)


class DeviceBraTS:
    """Training batches (x, target, edge, missing_modal [B,4] bool) prepared on `device` by prepare_batch: one HIP launch per eight
    samples for crop + flips + intensity + label remap + edge codes, written straight into caller-owned buffers with out=.

    source: a directory of .npz subjects (NpzBraTS's layout; `list_file` as NpzBraTS's) or a list of (image, label) pairs -- e.g.
    utils.synthetic.synthetic_volume outputs.  Sample i of epoch e uses draw_params(seed, e, i, its extents, crop, flip, intensity,
    rotate, scale, elastic, elastic_grid); with augmentation off a batch equals torch.stack of NpzBraTS / SyntheticBraTS items.
    rotate (degrees) / scale > 0 turn the crop into a randomly rotated / zoomed one (trilinear image, nearest label) in the same
    launch; elastic (voxels) > 0 deforms it by a cubic B-spline of elastic_grid^3 control displacements ~ U(-elastic, elastic).
    blur (largest sigma, 0.5..1.5) / noise (largest sigma) / gamma (half-width of the exponent's range about 1) > 0 switch the
    intensity stage on per channel (draw_params), which runs on the prepared crop in launches of its own.
    bias (half-width of the log multiplier, with bias_grid^3 control points) / contrast (half-width of the factor's range about 1) /
    lowres (smallest zoom of the coarse lattice, 0.5 <= z < 1) > 0 switch the acquisition stage on per channel, which runs between
    the two: bias field, contrast, low-resolution simulation (_acquisition_stage_cpu).
      cache=True   every subject is loaded once onto the device (fp32 image, uint8 label, optionally z-scored by normalize_nonzero)
      cache=False  "staged": NpzCropSource crops in DataLoader workers (batches()), the crops are uploaded from pinned memory and
                   prepared at origin 0 -- 36 MB per 128^3 sample over the host link instead of a whole subject.  With rotate /
                   scale / elastic the workers cut staged_box, the part of the volume the resampled crop reads, and the origin moves with it:
                   the batch is bit-equal to cache=True.
    oversample p > 0 (nnU-Net's oversample_foreground_percent; 0.33 there) moves that share of the crops onto a voxel of a randomly
    chosen non-empty region of foreground_regions (class bitmasks, default classes 1, 2, 3), taken from the subject's class_locations
    table of foreground_samples entries per region (draw_params, foreground_origin).  The tables are built once at construction, on
    `device`: with cache=True from the cached labels into one [n, R, K] / [n, R] tensor pair that is copied to the host once, after
    the last subject; with cache=False from each subject's label alone (the only array read), which is dropped again.  With p = 0
    no table is built and nothing new is called.
    crop_nonzero (what nnU-Net gets from cropping every subject to its nonzero box in preprocessing; off by default, and then nothing
    new is called) draws the origins that are not foreground origins inside the subject's nonzero box (draw_params(box=),
    box_crop_origin): the crop lies in the box, or the box in the crop.  The box is that of the raw image, before normalize.  With
    cache=True on a GPU it is one cwf_nonzero_box call per subject at construction into one [n, 6] tensor that is copied to the host
    once, after the last subject; otherwise (staged mode, a CPU instance) NpzCropSource takes it with numpy from the image it has
    just loaded, DataLoader workers included.  All of them give bit-equal batches; a subject that is zero everywhere is drawn as if
    the option were off."""

    def __init__(self, source, device, crop=(128, 128, 128), seed=1000, flip=False, intensity=0.0, normalize=False, cache=True,
                 list_file=None, rotate=0.0, scale=0.0, elastic=0.0, elastic_grid=7, blur=0.0, noise=0.0, gamma=0.0, bias=0.0,
                 bias_grid=4, contrast=0.0, lowres=0.0, oversample=0.0, foreground_regions=FOREGROUND_CLASSES, foreground_samples=4096,
                 crop_nonzero=False):
        self.device = torch.device(device)
        self.crop_nonzero = bool(crop_nonzero)
        self.crop, self.seed, self.epoch = tuple(int(c) for c in crop), int(seed), 0
        self.flip, self.intensity, self.normalize, self.cache = bool(flip), float(intensity), bool(normalize), bool(cache)
        self.rotate, self.scale = float(rotate), float(scale)
        self.elastic, self.elastic_grid = float(elastic), int(elastic_grid)
        self.blur, self.noise, self.gamma = float(blur), float(noise), float(gamma)
        self.bias, self.bias_grid, self.contrast, self.lowres = float(bias), int(bias_grid), float(contrast), float(lowres)
        if self.bias > 0.0 and not ELASTIC_GRID_MIN <= self.bias_grid <= ELASTIC_GRID_MAX:
            raise ValueError("DeviceBraTS: bias_grid takes %d..%d control points per axis" % (ELASTIC_GRID_MIN, ELASTIC_GRID_MAX))
        if self.elastic > 0.0 and not ELASTIC_GRID_MIN <= self.elastic_grid <= ELASTIC_GRID_MAX:
            raise ValueError("DeviceBraTS: elastic_grid takes %d..%d control points per axis" % (ELASTIC_GRID_MIN, ELASTIC_GRID_MAX))
        self.affine = self.rotate > 0.0 or self.scale > 0.0 or self.elastic > 0.0      # the crop is resampled
        subjects = _npz_paths(source, list_file) if isinstance(source, str) else list(source)
        if not subjects:
            raise ValueError("DeviceBraTS: no subjects")
        self.source = NpzCropSource(subjects, self.crop, self.seed, self.normalize, self.flip, self.intensity, self.rotate, self.scale,
                                    self.elastic, self.elastic_grid, crop_nonzero=self.crop_nonzero)
        self.images = self.labels = None
        self.oversample, self.foreground = float(oversample), None
        if not 0.0 <= self.oversample <= 1.0:
            raise ValueError("DeviceBraTS: oversample takes a probability in [0, 1], got %r" % (oversample,))
        if self.oversample > 0.0:
            self.foreground_regions, self.foreground_samples = _check_regions(foreground_regions, foreground_samples)
        if self.cache:
            self._load_all(subjects)
        if self.oversample > 0.0:
            self.foreground = self._locate_all()
            self.source.oversample, self.source.foreground = self.oversample, self.foreground

    def _load_all(self, subjects):
        if self.device.type == "cuda":
            need = 0
            for s in subjects:
                if isinstance(s, str):
                    ishape, lshape = _npz_shapes(s)
                else:
                    ishape, lshape = tuple(s[0].shape), tuple(s[1].shape)
                need += 4 * int(np.prod(ishape)) + int(np.prod(lshape))
            free, _ = torch.cuda.mem_get_info(self.device)
            if need > 0.9 * free:
                raise MemoryError("DeviceBraTS(cache=True) needs %.1f GB of device memory for %d subjects, %.1f GB are free: use "
                                  "cache=False (the 'staged' mode) instead" % (need / 1e9, len(subjects), free / 1e9))
        self.images, self.labels = [], []
        boxes = None
        if self.crop_nonzero and self.device.type != "cpu":     # one row per subject, written by cwf_nonzero_box on the raw image
            boxes = torch.empty((len(subjects), 6), dtype=torch.int32, device=self.device)
            counts = torch.empty(len(subjects), dtype=torch.int64, device=self.device)
        for i in range(len(subjects)):
            img, lab = self.source.load(i) if self.device.type == "cpu" else \
                self._load_raw(i, None if boxes is None else (boxes[i:i + 1], counts[i:i + 1]))
            self.images.append(img)
            self.labels.append(lab)
        if boxes is not None:
            self.source.boxes = {i: tuple(int(v) for v in row) for i, row in enumerate(boxes.cpu().numpy())}

    def _locate_all(self):
        """the per-subject list of host (counts int64 [R], table int32 [R, K]) pairs: one class_locations call per subject into its
        rows of one tensor pair on the device, one copy to the host after the last"""
        n, R, K = len(self.source), len(self.foreground_regions), self.foreground_samples
        counts = torch.empty((n, R), dtype=torch.int64, device=self.device)
        table = torch.empty((n, R, K), dtype=torch.int32, device=self.device)
        for i in range(n):
            lab = self.labels[i] if self.labels is not None else self.source.load_label(i).to(self.device)
            if lab.is_cuda:
                from cwf import kernels
                kernels.backend().class_locations(lab.contiguous(), self.foreground_regions, K, out=(counts[i], table[i]))
            else:
                c, t = class_locations(lab, self.foreground_regions, K)
                counts[i], table[i] = c, t
        counts, table = counts.cpu().numpy(), table.cpu().numpy()
        return [(counts[i], table[i]) for i in range(n)]

    def _load_raw(self, i, box_out=None):
        """subject i on the device; normalised there (the device kernel) when asked.  box_out: the (box [1, 6], count [1]) rows that
        cwf_nonzero_box fills from the raw image"""
        src = self.source
        norm, src.normalize, nz, src.crop_nonzero = src.normalize, False, src.crop_nonzero, False
        try:
            img, lab = src.load(i)
        finally:
            src.normalize, src.crop_nonzero = norm, nz
        img, lab = img.to(self.device).contiguous(), lab.to(self.device).contiguous()
        if box_out is not None:
            from cwf import kernels
            kernels.backend().nonzero_box(img[None], out=box_out)
        if self.normalize:
            normalize_nonzero(img)
        return img, lab

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self.source.set_epoch(epoch)

    def __len__(self):
        return len(self.source)

    def extents(self, i):
        if self.labels is not None:
            return tuple(self.labels[i].shape)
        s = self.source.subjects[i]
        return tuple(_npz_shapes(s)[1]) if isinstance(s, str) else tuple(s[1].shape)

    def params(self, i):
        return draw_params(self.seed, self.epoch, i, self.extents(i), self.crop, self.flip, self.intensity, self.rotate, self.scale,
                           self.elastic, self.elastic_grid, self.blur, self.noise, self.gamma, self.bias, self.bias_grid, self.contrast,
                           self.lowres, **self.source._origin_keywords(i))

    def _missing(self, n):
        return torch.zeros((n, 4), dtype=torch.bool, device=self.device)

    def batch(self, indices, out=None):
        """(x, target, edge, missing) for the subjects `indices` in the current epoch."""
        indices = [int(i) for i in indices]
        if self.cache:
            x, t, e = prepare_batch([self.images[i] for i in indices], [self.labels[i] for i in indices],
                                    [self.params(i) for i in indices], self.crop, out=out)
            return x, t, e, self._missing(len(indices))
        return self.prepare_staged(_collate_crops([self.source[i] for i in indices], stack=not self.affine), out=out)

    def prepare_staged(self, crops, out=None):
        """(image crops [B,4,*crop] float32, label crops [B,*crop] uint8, indices) from NpzCropSource -> the prepared batch; with
        rotate / scale / elastic the crops are lists of source boxes and every sample is re-origined by its box's low corner"""
        imgs, labs, idx, *boxes = crops
        if boxes:                           # crop_nonzero: what the loader (a worker, perhaps) found for these subjects
            self.source.boxes.update((int(i), tuple(int(v) for v in b)) for i, b in zip(idx, boxes[0]))
        params = [self.params(i) for i in idx]
        if self.affine:
            if self.device.type == "cuda":
                imgs = [v.to(self.device, non_blocking=True) for v in imgs]
                labs = [v.to(self.device, non_blocking=True) for v in labs]
            params = [p.at_origin([o - b[0] for o, b in zip(p.origin, staged_box(p, self.extents(i), self.crop))])
                      for p, i in zip(params, idx)]
        else:
            if self.device.type == "cuda":
                imgs, labs = imgs.to(self.device, non_blocking=True), labs.to(self.device, non_blocking=True)
            params = [p.at_origin((0, 0, 0)) for p in params]
        x, t, e = prepare_batch(list(imgs), list(labs), params, self.crop, out=out)
        return x, t, e, self._missing(len(idx))

    def batches(self, index_batches, num_workers=0, out=None):
        """Yield batch(b) for each index list b; out may be a callable evaluated per batch (e.g. a Trainer's captured inputs, which
        exist only after the first steps).  A batch is prepared only when asked for, behind the work already on the stream."""
        index_batches = [list(b) for b in index_batches]
        get_out = out if callable(out) else (lambda: out)
        if self.cache:
            for b in index_batches:
                yield self.batch(b, out=get_out())
            return
        loader = torch.utils.data.DataLoader(self.source, batch_sampler=index_batches, num_workers=int(num_workers),
                                             collate_fn=_collate_crops if not self.affine else _collate_boxes,
                                             pin_memory=self.device.type == "cuda")
        for crops in loader:
            yield self.prepare_staged(crops, out=get_out())
