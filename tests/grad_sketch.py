"""Count-sketch of a parameter gradient: a fixture of 256 numbers per tensor that still pins every element.

Element ``i`` of a tensor (contiguous layout, ``n`` elements) goes to bucket ``h1(i) mod S`` with sign ``h2(i)`` in {-1, +1}; the
sketch is the ``S`` signed bucket sums in float64.  ``S = 256``; a tensor with ``n <= S`` is kept whole (``S := n``, identity map), so
biases, LayerNorm vectors and class tokens are compared element by element.  The hash is seeded with the tensor's index in the fixture's
``grad_names``: two tensors of one shape get different patterns, so exchanging them shows.

The distance is ``d = |sk(got) - sk(ref)|_2 / |sk(ref)|_2``.  With independent signs ``E|sk(e)|^2 = |e|^2`` for any ``e`` (the cross
terms of a bucket cancel in expectation) and the relative standard deviation of ``|sk(e)|^2`` is at most ``sqrt(2 / S)`` = 0.088, so the
ratio of two such estimates is off by about 6 % at one sigma in ``d``: ``ESTIMATOR_FACTOR`` = 1.25 is four sigma, and
test_grad_sketch_cpu.py counts how often real gradients leave it.

``_hash`` is the one place the hash is written: ``+ * ^ >> &`` on int64 with wrap-around, which numpy arrays and torch tensors (on any
device) evaluate identically.  ``>>`` on int64 is an arithmetic shift in both; every shift is masked down to the bits a logical shift
would keep.
"""
import numpy as np
import torch

S = 256
ESTIMATOR_FACTOR = 1.25          # four sigma of the estimator, see above


def _i64(v):
    """a Python integer reduced to the signed 64-bit value with the same bits"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


_C0, _C1, _C2 = _i64(0x9E3779B97F4A7C15), _i64(0xBF58476D1CE4E5B9), _i64(0x94D049BB133111EB)


def _hash(i, seed):
    """splitmix64's finaliser of ``i + (seed + 1) * C0`` on an int64 numpy array or torch tensor -> (bucket in [0, S), sign bit in {0, 1})"""
    z = i + _i64((seed + 1) * _C0)
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * _C1
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * _C2
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return (z & 0x7FFFFFFF) % S, (z >> 40) & 1


def pattern_np(n, seed, start=0):
    """(bucket int64 [n], sign float64 [n]) of elements start .. start + n - 1, numpy"""
    with np.errstate(over="ignore"):
        b, s = _hash(np.arange(start, start + n, dtype=np.int64), seed)
    return b, 1.0 - 2.0 * s.astype(np.float64)


def pattern_torch(n, seed, device, start=0):
    """the same pattern as torch tensors on ``device``"""
    b, s = _hash(torch.arange(start, start + n, dtype=torch.int64, device=device), seed)
    return b, 1.0 - 2.0 * s.to(torch.float64)


def sketch_np(a, seed):
    """float64 sketch of a numpy array: [min(n, S)]"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if a.size <= S:
        return a.copy()
    b, s = pattern_np(a.size, seed)
    return np.bincount(b, weights=a * s, minlength=S)


def sketch_torch(t, seed):
    """float64 sketch of a torch tensor, computed where the tensor lives (index_add_ into a float64 buffer): [min(n, S)]"""
    t = t.detach().contiguous().reshape(-1).to(torch.float64)
    if t.numel() <= S:
        return t.clone()
    b, s = pattern_torch(t.numel(), seed, t.device)
    return torch.zeros(S, dtype=torch.float64, device=t.device).index_add_(0, b, t * s)


def distance(got, ref):
    """d = |got - ref| / |ref| of two sketches (numpy)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def remove_orthogonal_component(g, frac, rng):
    """g = a + c with c orthogonal to a and |c| = frac |a|; returns a.  c is g's projection on a unit vector u at the angle to g whose
    cosine is frac / sqrt(1 + frac^2)."""
    flat = g.reshape(-1)
    v = rng.standard_normal(flat.size)
    gn = flat / np.linalg.norm(flat)
    v -= (v @ gn) * gn
    v /= np.linalg.norm(v)
    cos = frac / np.sqrt(1.0 + frac * frac)
    u = cos * gn + np.sqrt(1.0 - cos * cos) * v
    return (flat - (flat @ u) * u).reshape(g.shape)


# ---- the fixture (tests/golden/grads_*.npz, written by oracle/make_golden.py: gradient_sketches)

def pack_reference(names, grads64, grads32):
    """The fixture's gradient entries from the reference's float64 gradients (and its fp32 ones, for the noise floor in this metric).
    ``sketch_f64`` [len(names), S] holds a row per tensor (zero beyond a whole tensor's n); the whole tensors (n <= S) are also stored
    back to back in ``whole_f64`` with ``whole_offsets`` [len(names) + 1]."""
    sk = np.zeros((len(names), S))
    whole, off, noise, l2 = [], [0], [], []
    for i, n in enumerate(names):
        g = grads64[n].detach().double().numpy()
        r = sketch_np(g, i)
        sk[i, :r.size] = r
        if g.size <= S:
            whole.append(r)
        off.append(off[-1] + (g.size if g.size <= S else 0))
        l2.append(float(np.linalg.norm(g)))
        d = np.linalg.norm(sketch_np(grads32[n].detach().double().numpy(), i) - r)
        noise.append(float(d / (np.linalg.norm(r) + 1e-30)))
    return dict(grad_names=np.array(names), sketch_f64=sk, whole_f64=np.concatenate(whole), whole_offsets=np.array(off, dtype=np.int64),
                l2_f64=np.array(l2), noise_sketch=np.array(noise), numel=np.array([grads64[n].numel() for n in names], dtype=np.int64))


def reference_sketches(fx):
    """{name: (index, float64 sketch [min(n, S)])} of a loaded fixture; whole tensors come from the ragged array"""
    out = {}
    off = fx["whole_offsets"]
    for i, (n, numel) in enumerate(zip(fx["grad_names"], fx["numel"])):
        out[str(n)] = (i, fx["whole_f64"][off[i]:off[i + 1]] if numel <= S else fx["sketch_f64"][i])
    return out


def bound(noise, floor):
    """the tests' bound on d for a tensor whose reference-fp32 noise (in this metric) is ``noise``: the estimator's factor over
    max(10 x noise, floor), floor = the project's elementwise figure (1e-2; 2e-2 with single-bf16 gradient operands)"""
    return ESTIMATOR_FACTOR * max(10.0 * float(noise), floor)


LIVE_L2 = 1e-7        # at or below: a bias in front of an InstanceNorm, true gradient zero
DEAD_L2_MAX = 1e-5    # ... whose computed gradient (cancellation noise) must stay this small in norm


def check(fx, got, floor, dead_excused=()):
    """Hold gradients ``got`` {name: torch tensor, anywhere} to the fixture.  Returns (over, dead, worst): ``over`` lists
    (name, d, bound) of every live tensor beyond its bound and (name, norm, DEAD_L2_MAX) of every dead one above DEAD_L2_MAX that is
    not named in ``dead_excused``; ``dead`` = {name: norm} of the tensors not held to a bound; ``worst`` = (max d / bound over the live
    tensors, its name).  Asserts every gradient finite and every fixture name present."""
    refs = reference_sketches(fx)
    assert set(got) == set(refs), sorted(set(got) ^ set(refs))[:5]
    over, dead, worst = [], {}, (0.0, None)
    for n, (i, ref) in refs.items():
        g = got[n]
        assert g.numel() == int(fx["numel"][i]), n
        assert bool(torch.isfinite(g).all()), n
        if fx["l2_f64"][i] > LIVE_L2:
            d = distance(sketch_torch(g, i).cpu().numpy(), ref)
            b = bound(fx["noise_sketch"][i], floor)
            if d > b:
                over.append((n, d, b))
            if d / b > worst[0]:
                worst = (d / b, n)
        else:
            dead[n] = float(g.double().norm())
            if dead[n] > DEAD_L2_MAX and n not in dead_excused:
                over.append((n, dead[n], DEAD_L2_MAX))
    return over, dead, worst
