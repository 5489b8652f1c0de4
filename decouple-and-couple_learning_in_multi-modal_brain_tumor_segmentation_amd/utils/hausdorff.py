"""Drop-in for the reference's ``utils/hausdorff.py``: ``ConfusionMatrix``, ``hausdorff_distance`` and ``hausdorff_distance_95``
with the reference's signatures and wrapper rules, and medpy's ``hd`` / ``hd95`` computed on the device (``csrc/metrics.hip``,
``cwf_hausdorff``): border extraction, an exact float64 Euclidean distance transform and the order statistics all run in HIP, and
only the scalar results come back to the host.

``avg_surface_distance`` (medpy ``asd``), ``avg_surface_distance_symmetric`` (medpy ``assd``) and ``normalized_surface_dice`` follow
the same wrapper rules on the same borders and distances (``cwf_surface_metrics``).  These three run on the device for CUDA tensors
and with numpy + scipy for everything else.

Inputs are numpy arrays or torch tensors on any device (host inputs are moved to the current GPU); the results are Python floats.
The empty / full rules come from the masks alone, before any GPU call.

medpy works in the rank of the arrays it is given, and the reference's evaluation passes ``[1, H, W, D]`` arrays: the erosion footprint
then reaches along the singleton axis, out of the volume, so every mask voxel is a border voxel.  That is reproduced here:
  rank 3                                -> surface borders (mask minus its erosion)
  rank >= 4, every leading axis size 1  -> every mask voxel is a border voxel ("all-border")
  anything else                         -> ValueError
"""
import math

import numpy as np
import torch

_EMPTY_FIRST = "The first supplied array does not contain any binary object."
_EMPTY_SECOND = "The second supplied array does not contain any binary object."


def volume_mode(shape):
    """(all_border, (D0, D1, D2)) for an array shape under the rank rules above."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 3:
        return False, shape
    if len(shape) >= 4 and all(s == 1 for s in shape[:-3]):
        return True, shape[-3:]
    raise ValueError("Hausdorff metrics take a 3-D volume or [1, ..., 1, D0, D1, D2]; got shape %s" % (shape,))


def spacing3(voxel_spacing, ndim):
    """medpy's voxelspacing (None, a scalar or one value per axis of the ndim-D input) -> the spacing of the last three axes."""
    if voxel_spacing is None:
        return None
    if np.isscalar(voxel_spacing):
        return (float(voxel_spacing),) * 3
    sp = tuple(float(s) for s in voxel_spacing)
    if len(sp) != ndim:
        raise ValueError("voxel_spacing needs %d values (one per axis), got %d" % (ndim, len(sp)))
    return sp[-3:]


def _nonzero(x):
    return x != 0


def _device_mask(x):
    """A mask as a [1, D0, D1, D2] uint8 tensor on a GPU (the current one for host inputs)."""
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.to(torch.device("cuda", torch.cuda.current_device()))
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x) != 0)).to(torch.device("cuda", torch.cuda.current_device()))
    if t.dtype != torch.bool:
        t = t != 0
    return t.reshape((1,) + tuple(t.shape[-3:])).contiguous().view(torch.uint8)


def _device_labels(x, device):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(device=device, dtype=torch.int64).reshape((1,) + tuple(t.shape[-3:])).contiguous()


def hd_hd95(test, reference, voxel_spacing=None, connectivity=1):
    """medpy.metric.binary (hd, hd95) of two masks of one shape, as Python floats; RuntimeError (medpy's) if either is empty."""
    from cwf.kernels import backend
    if tuple(test.shape) != tuple(reference.shape):
        raise ValueError("Shape mismatch: %s and %s" % (tuple(test.shape), tuple(reference.shape)))
    all_border, _ = volume_mode(test.shape)
    sp = spacing3(voxel_spacing, len(test.shape))
    a = _device_mask(test)
    with torch.cuda.device(a.device):
        b = _device_mask(reference).to(a.device)
        hd, hd95, counts = backend().hausdorff(a, b, 1, spacing=sp, connectivity=connectivity, all_border=all_border)
        res = torch.cat([hd.reshape(-1), hd95.reshape(-1), counts.reshape(-1)[:2].double()]).cpu().tolist()
    if res[2] == 0:
        raise RuntimeError(_EMPTY_FIRST)
    if res[3] == 0:
        raise RuntimeError(_EMPTY_SECOND)
    return res[0], res[1]


def _any(x):
    return bool(x.any()) if isinstance(x, torch.Tensor) else bool(np.any(x))


def _all(x):
    return bool(x.all()) if isinstance(x, torch.Tensor) else bool(np.all(x))


class ConfusionMatrix:
    """The reference's ConfusionMatrix (tp / fp / tn / fn, size, empty / full flags) for numpy arrays or torch tensors."""

    def __init__(self, test=None, reference=None):
        self.tp = self.fp = self.tn = self.fn = None
        self.size = None
        self.reference_empty = self.reference_full = self.test_empty = self.test_full = None
        self.set_reference(reference)
        self.set_test(test)

    def set_test(self, test):
        self.test = test
        self.reset()

    def set_reference(self, reference):
        self.reference = reference
        self.reset()

    def reset(self):
        self.tp = self.fp = self.tn = self.fn = None
        self.size = None
        self.test_empty = self.test_full = self.reference_empty = self.reference_full = None

    def compute(self):
        if self.test is None or self.reference is None:
            raise ValueError("'test' and 'reference' must both be set to compute confusion matrix.")
        assert tuple(self.test.shape) == tuple(self.reference.shape), \
            "Shape mismatch: {} and {}".format(tuple(self.test.shape), tuple(self.reference.shape))
        t, r = _nonzero(self.test), _nonzero(self.reference)
        self.tp = int((t & r).sum())
        self.fp = int((t & ~r).sum())
        self.tn = int((~t & ~r).sum())
        self.fn = int((~t & r).sum())
        self.size = int(np.prod(tuple(self.reference.shape), dtype=np.int64))
        self.test_empty = not _any(t)
        self.test_full = _all(t)
        self.reference_empty = not _any(r)
        self.reference_full = _all(r)

    def get_matrix(self):
        if any(e is None for e in (self.tp, self.fp, self.tn, self.fn)):
            self.compute()
        return self.tp, self.fp, self.tn, self.fn

    def get_size(self):
        if self.size is None:
            self.compute()
        return self.size

    def get_existence(self):
        if any(e is None for e in (self.test_empty, self.test_full, self.reference_empty, self.reference_full)):
            self.compute()
        return self.test_empty, self.test_full, self.reference_empty, self.reference_full


def _wrapped(which, test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity):
    if confusion_matrix is None:
        confusion_matrix = ConfusionMatrix(test, reference)
    if confusion_matrix.test is not None:
        volume_mode(confusion_matrix.test.shape)
    test_empty, test_full, reference_empty, reference_full = confusion_matrix.get_existence()
    if test_empty or test_full or reference_empty or reference_full:
        return math.nan if nan_for_nonexisting else 0.0
    return hd_hd95(confusion_matrix.test, confusion_matrix.reference, voxel_spacing, connectivity)[which]


def hausdorff_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=False, voxel_spacing=None, connectivity=1,
                       **kwargs):
    """medpy's hd of the two masks; 0 (NaN with nan_for_nonexisting) when either mask is empty or full."""
    return _wrapped(0, test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity)


def hausdorff_distance_95(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=False, voxel_spacing=None, connectivity=1,
                          **kwargs):
    """medpy's hd95 of the two masks; 0 (NaN with nan_for_nonexisting) when either mask is empty or full."""
    return _wrapped(1, test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity)


def surface_host(a, b, tolerances=(), spacing=None, connectivity=1, all_border=False):
    """The surface metrics of two non-empty 3-D masks with scipy: (asd (2,), assd, within [T][2], nsd [T], (|dA|, |dB|)) as
    cwf_surface_metrics defines them, the means correctly rounded (math.fsum).  Computed on the bounding box of a | b grown by one
    voxel inside the volume (every border voxel of either mask lies in it, and what lies beyond it is unset in both)."""
    from scipy import ndimage
    box = tuple(slice(max(int(i.min()) - 1, 0), int(i.max()) + 2) for i in np.nonzero(a | b))
    a, b = a[box], b[box]
    if all_border:
        ba, bb = a, b
    else:
        fp = ndimage.generate_binary_structure(3, connectivity)
        ba, bb = a & ~ndimage.binary_erosion(a, structure=fp), b & ~ndimage.binary_erosion(b, structure=fp)
    sp = (1.0, 1.0, 1.0) if spacing is None else ((float(spacing),) * 3 if np.isscalar(spacing) else tuple(float(v) for v in spacing))
    da = ndimage.distance_transform_edt(~bb, sampling=sp)[ba]
    db = ndimage.distance_transform_edt(~ba, sampling=sp)[bb]
    asd = (math.fsum(da.tolist()) / da.size, math.fsum(db.tolist()) / db.size)
    within = [[int((da <= t).sum()), int((db <= t).sum())] for t in tolerances]
    nsd = [float(w[0] + w[1]) / float(da.size + db.size) for w in within]
    return asd, (asd[0] + asd[1]) / 2.0, within, nsd, (int(da.size), int(db.size))

def surface_stats(test, reference, tolerances=(), voxel_spacing=None, connectivity=1):
    """(asd(test, reference), asd(reference, test), assd, [nsd per tolerance]) of two masks of one shape as Python floats, under the
    rank rules above; RuntimeError (medpy's) if either is empty.  CUDA tensors run cwf_surface_metrics, everything else surface_host."""
    if tuple(test.shape) != tuple(reference.shape):
        raise ValueError("Shape mismatch: %s and %s" % (tuple(test.shape), tuple(reference.shape)))
    all_border, vol = volume_mode(test.shape)
    sp = spacing3(voxel_spacing, len(test.shape))
    tol = tuple(float(t) for t in tolerances)
    if isinstance(test, torch.Tensor) and test.is_cuda:
        from cwf.kernels import backend
        a = _device_mask(test)
        with torch.cuda.device(a.device):
            b = _device_mask(reference).to(a.device)
            out = backend().surface_metrics(a, b, 1, tol, spacing=sp, connectivity=connectivity, all_border=all_border)
            res = torch.cat([out["asd"].reshape(-1), out["assd"].reshape(-1), out["nsd"].reshape(-1),
                             out["counts"].reshape(-1)[:2].double()]).cpu().tolist()
        if res[-2] == 0:
            raise RuntimeError(_EMPTY_FIRST)
        if res[-1] == 0:
            raise RuntimeError(_EMPTY_SECOND)
        return res[0], res[1], res[2], res[3:3 + len(tol)]
    a = np.asarray(_nonzero(test.cpu() if isinstance(test, torch.Tensor) else np.asarray(test))).reshape(vol)
    b = np.asarray(_nonzero(reference.cpu() if isinstance(reference, torch.Tensor) else np.asarray(reference))).reshape(vol)
    if not a.any():
        raise RuntimeError(_EMPTY_FIRST)
    if not b.any():
        raise RuntimeError(_EMPTY_SECOND)
    asd, assd, _, nsd, _ = surface_host(a, b, tol, sp, connectivity, all_border)
    return asd[0], asd[1], assd, nsd


def _wrapped_surface(pick, test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, tolerances=()):
    if confusion_matrix is None:
        confusion_matrix = ConfusionMatrix(test, reference)
    if confusion_matrix.test is not None:
        volume_mode(confusion_matrix.test.shape)
    test_empty, test_full, reference_empty, reference_full = confusion_matrix.get_existence()
    if test_empty or test_full or reference_empty or reference_full:
        return math.nan if nan_for_nonexisting else 0.0
    return pick(surface_stats(confusion_matrix.test, confusion_matrix.reference, tolerances, voxel_spacing, connectivity))


def avg_surface_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=False, voxel_spacing=None, connectivity=1,
                         **kwargs):
    """medpy's asd(test, reference): the mean distance from the border voxels of test to the border of reference; 0 (NaN with
    nan_for_nonexisting) when either mask is empty or full."""
    return _wrapped_surface(lambda s: s[0], test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity)


def avg_surface_distance_symmetric(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=False, voxel_spacing=None,
                                   connectivity=1, **kwargs):
    """medpy's assd: the mean of asd(test, reference) and asd(reference, test); 0 (NaN with nan_for_nonexisting) when either mask is
    empty or full."""
    return _wrapped_surface(lambda s: s[2], test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity)


def normalized_surface_dice(test=None, reference=None, tolerance=1.0, confusion_matrix=None, nan_for_nonexisting=False, voxel_spacing=None,
                            connectivity=1, **kwargs):
    """The normalised surface Dice at `tolerance` (in voxel_spacing units): the share of the border voxels of both masks that lie
    within the tolerance of the other mask's border -- the voxel-border form, not the area-weighted surface-element one; with unit
    spacing a tolerance < 1 counts coincident border voxels only.  0 (NaN with nan_for_nonexisting) when either mask is empty or full."""
    if not float(tolerance) >= 0.0:
        raise ValueError("normalized_surface_dice: tolerance must be >= 0 (and not NaN), got %r" % (tolerance,))
    return _wrapped_surface(lambda s: s[3][0], test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity,
                            (float(tolerance),))


def softmax_hd(output, target):
    """medpy's hd of the [WT, TC, ET] regions of two integer label maps (one launch set for all three); RuntimeError with medpy's
    message, in medpy's order, when a region is empty.  Host inputs are checked before any GPU call."""
    from cwf.kernels import backend
    if tuple(output.shape) != tuple(target.shape):
        raise ValueError("Shape mismatch: %s and %s" % (tuple(output.shape), tuple(target.shape)))
    all_border, _ = volume_mode(output.shape)
    on_device = isinstance(output, torch.Tensor) and output.is_cuda
    if not on_device:
        for o, t in zip(_regions(output), _regions(target)):
            if not _any(o):
                raise RuntimeError(_EMPTY_FIRST)
            if not _any(t):
                raise RuntimeError(_EMPTY_SECOND)
    dev = output.device if on_device else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        be = backend()
        a = be.region_bits(_device_labels(output, dev))
        b = be.region_bits(_device_labels(target, dev))
        hd, _, counts = be.hausdorff(a, b, 3, all_border=all_border)
        hd, counts = hd.reshape(3).cpu().tolist(), counts.reshape(3, 4).cpu().tolist()
    for r in range(3):
        if counts[r][0] == 0:
            raise RuntimeError(_EMPTY_FIRST)
        if counts[r][1] == 0:
            raise RuntimeError(_EMPTY_SECOND)
    return hd


def _regions(x):
    """[WT, TC, ET] masks of tools.softmax_output_dice."""
    return [x > 0, (x == 1) | (x == 3), x == 3]
