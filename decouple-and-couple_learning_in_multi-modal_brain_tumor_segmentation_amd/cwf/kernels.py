"""Tensor-level wrappers over the C ABI (include/cwf_hip.h).  torch is used for device memory and the current
stream only; every arithmetic op below is a launch of a hand-written gfx950 kernel.  There is no fallback:
constructing HipBackend without the built library or without a GPU raises.

Activation tensors are 5-D [N, D, H, W, C] with unit channel stride; a channel slice of a dense buffer is
passed zero-copy as (data_ptr, ldc = stride(3)).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import threading

import numpy as np
import torch

from . import _lib
from . import packing as pk

_f32 = torch.float32
# the evaluation's regions as class bitmasks (bit c = class c belongs): WT = {1, 2, 3}, TC = {1, 3}, ET = {3}
REGION_MASKS = (0b1110, 0b1010, 0b1000)
# the focal Tversky / focal cross-entropy term's parameters (struct cwf_focal_params) at their defaults
FOCAL_DEFAULTS = dict(fn=0.7, fp=0.3, exponent=0.75, smooth=1e-5, gamma=2.0, ce_ratio=1.0, class_weight=(1.0, 1.0, 1.0, 1.0))


def check_focal_params(posmasks, fn=0.7, fp=0.3, exponent=0.75, smooth=1e-5, gamma=2.0, ce_ratio=1.0, class_weight=None):
    """The accepted values of the focal term (the rules cwf_focal_loss enforces, here as ValueError before anything is called):
    at most 8 regions, each a non-zero bitmask over classes 0..3; fn, fp finite >= 0 with fn + fp > 0; 0 < exponent <= 4; smooth > 0;
    gamma = 0 or 1 <= gamma <= 5; ce_ratio finite >= 0; four class weights finite >= 0; not both parts off.  -> the parameters as a
    dict of floats (class_weight a 4-tuple)."""
    masks = tuple(int(m) for m in posmasks)
    if len(masks) > 8:
        raise ValueError("focal loss: at most 8 regions, got %d" % len(masks))
    if any(m <= 0 or m > 15 for m in masks):
        raise ValueError("focal loss: a region is a non-zero bitmask over classes 0..3, got %r" % (posmasks,))
    fn, fp, exponent, smooth, gamma, ce_ratio = (float(v) for v in (fn, fp, exponent, smooth, gamma, ce_ratio))
    if not (math.isfinite(fn) and math.isfinite(fp) and fn >= 0.0 and fp >= 0.0 and fn + fp > 0.0):
        raise ValueError("focal loss: fn and fp must be finite and >= 0 with fn + fp > 0, got %r and %r" % (fn, fp))
    if not 0.0 < exponent <= 4.0:
        raise ValueError("focal loss: exponent must lie in (0, 4], got %r" % (exponent,))
    if not (math.isfinite(smooth) and smooth > 0.0):
        raise ValueError("focal loss: smooth must be finite and > 0, got %r" % (smooth,))
    if not (gamma == 0.0 or 1.0 <= gamma <= 5.0):
        raise ValueError("focal loss: gamma must be 0 or lie in [1, 5] (a gamma in (0, 1) gives 0 * inf at p = 1), got %r" % (gamma,))
    if not (math.isfinite(ce_ratio) and ce_ratio >= 0.0):
        raise ValueError("focal loss: ce_ratio must be finite and >= 0, got %r" % (ce_ratio,))
    kw = (1.0, 1.0, 1.0, 1.0) if class_weight is None else tuple(float(k) for k in class_weight)
    if len(kw) != 4 or not all(math.isfinite(k) and k >= 0.0 for k in kw):
        raise ValueError("focal loss: class_weight must be four finite numbers >= 0, got %r" % (class_weight,))
    if not masks and ce_ratio == 0.0:
        raise ValueError("focal loss: both parts are off (no region and ce_ratio = 0)")
    return dict(fn=fn, fp=fp, exponent=exponent, smooth=smooth, gamma=gamma, ce_ratio=ce_ratio, class_weight=kw)


# the Lovasz-Softmax term's default regions: the four classes, one bitmask each (Lovasz-Softmax proper)
CLASS_MASKS = (1, 2, 4, 8)


def check_lovasz_params(posmasks, only_present=True):
    """The accepted values of the Lovasz-Softmax term (the rules cwf_lovasz enforces, here as ValueError before anything is called):
    1 to 8 regions, each a bitmask in 1..15 over classes 0..3; only_present a bool.  -> (the masks as a tuple of ints, only_present)"""
    try:
        masks = tuple(int(m) for m in posmasks)
    except TypeError:
        raise ValueError("lovasz: posmasks must be a sequence of class bitmasks, got %r" % (posmasks,))
    if not 1 <= len(masks) <= 8:
        raise ValueError("lovasz: 1 to 8 regions, got %d" % len(masks))
    if any(m < 1 or m > 15 for m in masks) or any(float(m) != float(q) for m, q in zip(masks, posmasks)):
        raise ValueError("lovasz: a region is a bitmask in 1..15 over classes 0..3, got %r" % (posmasks,))
    if not isinstance(only_present, (bool, np.bool_)):
        raise ValueError("lovasz: only_present must be True or False, got %r" % (only_present,))
    return masks, bool(only_present)


def cl(t: torch.Tensor):
    """(tensor, ldc) of a channels-last activation usable by the kernels; copies only if the strides are unusable."""
    assert t.dim() == 5 and t.dtype == _f32, (t.shape, t.dtype)
    n, d, h, w, c = t.shape
    s = t.stride()
    ldc = s[3]
    ok = s[4] == 1 and ldc >= c and ldc % 4 == 0 and s[2] == w * ldc and s[1] == h * w * ldc and s[0] == d * h * w * ldc \
        and t.data_ptr() % 16 == 0
    if not ok:
        t = t.contiguous()
        ldc = c
        if c % 4:
            raise ValueError("channel count must be a multiple of 4 for a copied activation")
    return t, ldc


def _p(t):
    return 0 if t is None else t.data_ptr()


def _tab(ts):
    """pointer table (up to 4 groups) for the grouped kernel forms"""
    return (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [0] * (4 - len(ts))))


def _ln_params(**kw):
    """struct cwf_ln_group_params from tensors or lists of tensors; returns (struct, groups)"""
    P = _lib.LnGroupParams()
    G = 1
    for name, v in kw.items():
        if v is None:
            continue
        vs = v if isinstance(v, (list, tuple)) else [v]
        G = max(G, len(vs))
        setattr(P, name, _tab(vs))
    return P, G


# Arithmetic of the conv family (forward, data gradient, weight gradient).  Activations / weights are fp32 in HBM in
# every mode; the mode selects the MFMA operand form:
#   "fp32"   v_mfma_f32_16x16x4_f32, exact f32 (the parity reference mode)
#   "bf16x3" split-bf16: hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16, fp32 accumulate (~2^-16 per product)
#   "bf16"   single bf16 product (2^-9 per product)
_PRECISION = "fp32"
_WGRAD_PRECISION = None      # None = follow _PRECISION; "bf16" = single-bf16 products for the weight gradients only (see set_precision)
_DGRAD_PRECISION = None      # the same for the data-gradient convolutions


# Debug switch (read at every call): in_bwd_apply16(..., need_f32=False) fills the fp32 carrier it leaves unwritten with NaN, so a
# consumer that reads it after all -- a graph whose single-consumer declaration is false -- shows up as a non-finite gradient.
POISON_UNWRITTEN_CARRIERS = False


def set_precision(mode: str, wgrad: str = None, dgrad: str = None):
    """`wgrad` / `dgrad` optionally select the operand form of the weight-gradient / data-gradient kernels alone ("bf16": one
    bf16 product, fp32 accumulate -- the usual mixed-precision choice for gradients), leaving the forward in `mode`."""
    global _PRECISION, _WGRAD_PRECISION, _DGRAD_PRECISION
    ok = ("fp32", "bf16x3", "bf16")
    if mode not in ok or wgrad not in (None,) + ok or dgrad not in (None,) + ok:
        raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
    for o in (wgrad, dgrad):
        if o is not None and (mode == "fp32") != (o == "fp32"):
            raise ValueError("the fp32 and the bf16 kernel families use different weight packings; choose all from one family")
    _PRECISION, _WGRAD_PRECISION, _DGRAD_PRECISION = mode, wgrad, dgrad


def precision() -> str:
    return _PRECISION


_raw_stream = torch._C._cuda_getCurrentRawStream
_current_device = torch._C._cuda_getDevice


def _priority_stream(device, which):
    """A stream of the lowest ("low") / highest ("high") priority the HIP runtime offers ("normal": torch's default pool).
    torch.cuda.Stream.priority_range() reports (0, -1) on ROCm -- no low priority -- so "low" goes to the runtime directly."""
    if which == "normal":
        return torch.cuda.Stream(device=device)
    if which == "high":
        return torch.cuda.Stream(device=device, priority=torch.cuda.Stream.priority_range()[1])
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    least, greatest = ctypes.c_int(0), ctypes.c_int(0)
    with torch.cuda.device(device):
        if hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) != 0 or least.value <= 0:
            return torch.cuda.Stream(device=device, priority=torch.cuda.Stream.priority_range()[1])   # no low level: any non-default pool
        h = ctypes.c_void_p()
        if hip.hipStreamCreateWithPriority(ctypes.byref(h), ctypes.c_uint(1), ctypes.c_int(least.value)) != 0:   # 1 = hipStreamNonBlocking
            raise RuntimeError("hipStreamCreateWithPriority failed")
    return torch.cuda.ExternalStream(h.value, device=device)


class HipBackend:
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CwfError("no GPU visible: the cwf kernels are gfx950-only and there is no CPU fallback")
        self._ws = {}
        self._arena = {}
        self._arena_off = {}
        self._rng = {}                         # device -> int64[2] {seed, step} (device-resident generator state)
        self._rng_seed = {}
        self._site = 0                         # per-step dropout-site offset (reset by begin_step, static across steps)
        self._wg_stream = {}                   # device -> side stream for weight gradients (opt-in, see wgrad_stream)
        self._wg_part = {}                     # layer key -> persistent split-K slab buffer (wgrad_to)
        self._wg_pending = []                  # descriptor rows awaiting the batched reduce (wgrad_flush)
        self._wg_held = []                     # launches held back while wgrad_defer is set (wgrad_release)
        self._wg_keep = []                     # operands of released launches, referenced until join_wgrad_stream
        self._wg_sync_needed = False           # a main-stream launch queued slabs: the side-stream reduce must wait for it (wgrad_flush)
        self._zero16 = {}                      # device -> 64 zero bytes, the halo source of the LDS-DMA kernels (zero16)
        self.flush_every_default = 10
        self.flush_every = self.flush_every_default
        self.wgrad_defer = False
        self._wg_tables = {}
        self.wgrad_async = False
        self._rng_lock = threading.Lock()      # the autograd engine may call in from its own thread

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _stream():
        # raw hipStream_t of the current torch stream.  torch.cuda.current_stream() costs ~8 us of Python per call (device
        # index resolution, os.environ look-ups) -- with ~470 launches per forward that was 10 % of the host time.
        return _raw_stream(_current_device())

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise _lib.CwfError("%s failed with status %d" % (name, rc))

    def workspace(self, key, nfloats, device):
        """Grow-only scratch buffers (wgrad partial slabs), one per (device, stream): reuse is stream-ordered."""
        # (buffers allocated while capturing live in the graph's private pool: keep them apart from the eager ones)
        k = (key, device, _raw_stream(_current_device()), torch.cuda.is_current_stream_capturing())
        buf = self._ws.get(k)
        if buf is None or buf.numel() < nfloats:
            buf = torch.empty(int(nfloats), dtype=_f32, device=device)
            self._ws[k] = buf
        return buf

    # Small f64 accumulators (InstanceNorm / loss sums) come from ONE arena that is zeroed once per step (begin_step, called
    # by the model's forward) instead of ~340 separate fill launches.  Regions are handed out once per step and never reused
    # within it; the arena is sized for forward + backward of a step with a generous margin and falls back to torch.zeros.
    ARENA_DOUBLES = 1 << 20

    # ------------------------------------------------------------------ dropout generator (K12)
    def rng(self, device):
        """Device generator state {seed, step}.  The seed follows torch.initial_seed(); the step word is advanced by a kernel
        in begin_step, so that a captured step draws fresh masks on every replay."""
        device = torch.device(device)
        st = self._rng.get(device)
        seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF
        if st is None or (self._rng_seed.get(device) != seed and not torch.cuda.is_current_stream_capturing()):
            st = torch.tensor([seed, 0], dtype=torch.int64, device=device)
            self._rng[device] = st
            self._rng_seed[device] = seed
        return st

    def rng_site(self, n):
        """Counter offset of a dropout site of n elements (two chained masks may be drawn: 2n counters)."""
        with self._rng_lock:
            off = self._site
            self._site = off + 2 * int(n)
        return off

    def begin_step(self, device):
        self._call("cwf_rng_advance", self.rng(device).data_ptr(), self._stream())
        self._site = 0
        a = self._arena.get(device)
        if a is None:
            a = torch.zeros(self.ARENA_DOUBLES, dtype=torch.float64, device=device)
            self._arena[device] = a
        else:
            a.zero_()
        self._arena_off[device] = 0

    def _zeros_f64(self, shape, device):
        n = 1
        for s in shape:
            n *= s
        device = torch.device(device)
        a = self._arena.get(device)
        if a is not None:
            off = self._arena_off[device]
            if off + n <= a.numel():
                self._arena_off[device] = off + ((n + 1) // 2) * 2         # keep 16-byte alignment
                return a[off:off + n].view(shape)
        return torch.zeros(shape, dtype=torch.float64, device=device)

    # ------------------------------------------------------------------ K1
    def conv(self, op, x, wpk, bias, cout, in_scale=None, in_shift=None, slope=1.0, residual=None, out_scale=None,
             stats=None, out=None, w_ref=None, out_channels_alloc=None, fwd_op=None, prec=None, nb=None, bias_ref=None, x16=None, y16=None):
        """Returns the output buffer.  With out_channels_alloc > cout the buffer has zero-filled padding channels
        (2-channel heads live in 4-channel tensors so that every later kernel sees 16-byte voxel rows).
        The library chooses the kernel (cwf_conv).  w_ref / bias_ref are the original parameters (tuples for a fused layer); a forward
        launch (fwd_op None) hands a single contiguous w_ref over as the raw weight, which the stem and first down-sampling kernels read."""
        x, x_ldc = cl(x)
        n, di, hi, wi, cin = x.shape
        if op == pk.CONV3_S2_DGRAD or op == pk.CONVT2_DGRAD:
            assert out is not None, "dgrad ops need an explicit output (its extent is not implied)"
        if out is None:
            do, ho, wo = pk.out_dims(op, di, hi, wi)
            ca = out_channels_alloc or cout
            # padding channels (2-channel head logits in 4-channel rows) are NOT initialised: every consumer of such a tensor reads
            # channels [0, cout) only (upsample_softmax, cwf_head_loss_*); the GRADIENT tensors of the same shape are written with
            # zero padding by their producers, because the data-gradient conv does read all allocated channels
            out = torch.empty((n, do, ho, wo, ca), dtype=_f32, device=x.device)
        y = out
        _, do, ho, wo, _ = y.shape
        mode = prec or ((_DGRAD_PRECISION or _PRECISION) if (fwd_op is not None) else _PRECISION)
        a = _lib.ConvArgs(op=op, precision=_lib.PRECISION[mode], x=x.data_ptr(), x_ldc=x_ldc, wpk=wpk.data_ptr(), bias=_p(bias),
                          y=y.data_ptr(), y_ldc=y.stride(3), in_scale=_p(in_scale), in_shift=_p(in_shift), in_slope=float(slope),
                          out_scale=_p(out_scale), stats=_p(stats), nb_slope=1.0,
                          N=n, Di=di, Hi=hi, Wi=wi, Cin=cin, Do=do, Ho=ho, Wo=wo, Cout=cout)
        if residual is not None:
            residual, a.r_ldc = cl(residual)
            a.residual = residual.data_ptr()
        if nb is not None:
            # data gradient whose output feeds the backward of act(IN(nb_x)): stats := (S1, S2) of that backward (see in_bwd_fused)
            nb_x, nb_scale, nb_shift, a.nb_slope = nb
            nb_x, a.nb_ldc = cl(nb_x)
            a.nb_x, a.nb_scale, a.nb_shift = nb_x.data_ptr(), nb_scale.data_ptr(), nb_shift.data_ptr()
        if x16 is not None:
            # the input as a bf16 image (bf16_dgrad_ok): x itself is not read
            assert x16.dtype == torch.bfloat16 and x16.is_contiguous() and tuple(x16.shape) == (n, di, hi, wi, cin)
            a.x16, a.zero16 = x16.data_ptr(), self.zero16(x.device).data_ptr()
        if y16 is not None:
            # the output also as a bf16 image (y16 [N,D,H,W,cout] bfloat16)
            assert y16.dtype == torch.bfloat16 and y16.is_contiguous()
            a.y16 = y16.data_ptr()
        if fwd_op is None and torch.is_tensor(w_ref) and w_ref.is_contiguous() and w_ref.dtype == _f32:
            a.w_raw = w_ref.data_ptr()             # (the stem and the first down-sampling layer read the raw weight)
        self._call("cwf_conv", ctypes.addressof(a), self._stream())
        return y

    def supports_fused_norm_bwd(self, prec=None):
        """The split-bf16 conv kernels can accumulate the InstanceNorm-backward sums in the data-gradient epilogue."""
        return (prec or _PRECISION) != "fp32"

    def in_bwd_apply(self, dy, x, scale, shift, slope, sums, dx_add=None):
        """Second half of in_bwd, given the (S1, S2) sums (from the data-gradient epilogue, conv(..., nb=...))."""
        dy, dy_ldc = cl(dy)
        x, x_ldc = cl(x)
        n, d, h, w, c = x.shape
        dx = torch.empty((n, d, h, w, c), dtype=_f32, device=x.device)
        a_ldc = 0
        if dx_add is not None:
            dx_add, a_ldc = cl(dx_add)
        self._call("cwf_in_bwd_apply", dy.data_ptr(), dy_ldc, x.data_ptr(), x_ldc, scale.data_ptr(), shift.data_ptr(), float(slope),
                   sums.data_ptr(), _p(dx_add), a_ldc, dx.data_ptr(), c, n, d * h * w, c, self._stream())
        return dx

    # ------------------------------------------------------------------ bf16 operand images (16-channel full-resolution layers)
    # The weight gradient of the full-resolution 16-channel 3x3x3 layers takes its operands as bf16 tensors [N,D,H,W,16] when both
    # exist (wgrad16d_kernel: LDS-DMA staging, half the bytes, no conversion): xa16 = bf16(act(IN(x))) is a side output of the
    # layer's own InstanceNorm-backward apply pass, dy16 of the pass that produced the incoming gradient.  Same operand values as
    # the fp32-tensor kernel computes per tile (single-bf16 products), so results do not change.
    # which bf16 images the main-stream InstanceNorm-backward apply pass (and the block tail) write as side outputs: each costs the
    # main stream 2 B per element; without it a conversion pass in front of the weight gradient costs the side stream 6 B per
    # element.  Measured (plan mode, one box, volumes/s): none 102.7, dx 104.2, xa,dx 106.2.
    APPLY_EMITS = ("xa", "dx")

    def bf16_operands_ok(self, op, cin, cout, nvox):
        if op != pk.CONV3_S1 or (_WGRAD_PRECISION or _PRECISION) != "bf16":
            return 0
        if cin == 16 and cout == 16 and nvox >= 32768:
            return 16                                      # wgrad16d_kernel
        if cin >= 32 and cin % 16 == 0 and cout % 32 == 0:
            return 32                                      # wgrad_s1d_kernel (32-channel output groups)
        return 0

    def bf16_dgrad_ok(self, op, cin, cout, shape):
        """the data gradient of such a layer (cin -> cout, output [n, d, h, w, cout] = shape) can read its incoming gradient as a bf16 image
        (conv(..., x16=)): the library's own answer for that launch, whose input channels are the forward layer's outputs"""
        if op != pk.CONV3_S1 or (_DGRAD_PRECISION or _PRECISION) != "bf16":
            return False
        n, d, h, w = shape[:4]
        return bool(self.lib.cwf_conv_x16_ok(op, n, d, h, w, cout, cin))

    def zero16(self, device):
        device = torch.device(device)
        t = self._zero16.get(device)
        if t is None:
            t = self._zero16[device] = torch.zeros(64, dtype=torch.uint8, device=device)
        return t

    def in_bwd_apply16(self, dy, x, scale, shift, slope, sums, dx_add=None, want_dx16=False, want_xa16=False, need_f32=True):
        """in_bwd_apply with the bf16 side outputs: returns (dx, dx16, xa16).  dx16 = bf16(dx); xa16 = bf16(act(x*scale+shift)).
        need_f32=False: dx is an UNWRITTEN carrier (nothing reads the fp32 gradient; autograd wants an fp32 tensor of x's shape)."""
        dy, dy_ldc = cl(dy)
        x, x_ldc = cl(x)
        n, d, h, w, c = x.shape
        dx = torch.empty((n, d, h, w, c), dtype=_f32, device=x.device)
        if not need_f32 and POISON_UNWRITTEN_CARRIERS:
            dx.fill_(float("nan"))
        dx16 = torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=x.device) if want_dx16 else None
        xa16 = torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=x.device) if want_xa16 else None
        assert need_f32 or dx16 is not None
        a_ldc = 0
        if dx_add is not None:
            dx_add, a_ldc = cl(dx_add)
        self._call("cwf_in_bwd_apply_ex", dy.data_ptr(), dy_ldc, x.data_ptr(), x_ldc, scale.data_ptr(), shift.data_ptr(), float(slope),
                   sums.data_ptr(), _p(dx_add), a_ldc, dx.data_ptr() if need_f32 else 0, c, _p(dx16), _p(xa16), n, d * h * w, c, self._stream())
        return dx, dx16, xa16

    def to_bf16(self, x, scale=None, shift=None, slope=1.0, out=None):
        """bf16(act(x*scale+shift)) (scale None: bf16(x)) as a [N,D,H,W,C] bfloat16 tensor -- a stream pass, for operands no producer emitted."""
        x, x_ldc = cl(x)
        n, d, h, w, c = x.shape
        y = out if out is not None else torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=x.device)
        assert y.dtype == torch.bfloat16 and y.is_contiguous() and tuple(y.shape) == (n, d, h, w, c)
        self._call("cwf_to_bf16", x.data_ptr(), x_ldc, _p(scale), _p(shift), float(slope), y.data_ptr(), n, d * h * w, c, self._stream())
        return y

    def to_bf16_side(self, x, scale, shift, slope):
        if not self.wgrad_async:
            return self.to_bf16(x, scale, shift, slope)
        with self._on_side_stream(x.device, x, scale, shift):
            y = self.to_bf16(x, scale, shift, slope)
        y.record_stream(torch.cuda.current_stream(x.device))      # (consumed on the side stream; freed by whoever drops the last reference)
        return y

    def conv_grouped(self, x_all, cin, wpks, biases, cout, y_all, x_goff, y_goff, w_refs=None, fwd_op=None, prec=None):
        """G = len(wpks) channel-grouped 3x3x3 stride-1 convs in ONE launch (cwf_conv with groups): group q reads channels
        [q*x_goff, q*x_goff + cin) of x_all and writes channels [q*y_goff, q*y_goff + cout) of y_all (same voxel rows).  Data
        gradients: pass the transposed packed weights (spec.packed(True)) and fwd_op.  Exact-fp32 mode: one launch per group."""
        x_all, x_ldc = cl(x_all)
        y, y_ldc = cl(y_all)
        n, d, h, w, _ = x_all.shape
        G = len(wpks)
        mode = prec or ((_DGRAD_PRECISION or _PRECISION) if (fwd_op is not None) else _PRECISION)
        a = _lib.ConvArgs(op=pk.CONV3_S1, precision=_lib.PRECISION[mode], x=x_all.data_ptr(), x_ldc=x_ldc, y=y.data_ptr(), y_ldc=y_ldc,
                          in_slope=1.0, nb_slope=1.0, groups=G, x_goff=x_goff, y_goff=y_goff,
                          N=n, Di=d, Hi=h, Wi=w, Cin=cin, Do=d, Ho=h, Wo=w, Cout=cout)
        for q in range(G):
            a.wpk_g[q] = wpks[q].data_ptr()
            a.bias_g[q] = 0 if biases is None else _p(biases[q])
        self._call("cwf_conv", ctypes.addressof(a), self._stream())
        return y_all


    # Weight gradients are leaves of the backward pass (only the optimizer reads them) while the data gradients form its
    # critical path.  With `wgrad_async` (opt-in: the caller must call join_wgrad_stream() before reading any .grad -- the
    # Trainer does) the weight-gradient kernels and their slab reductions go to a side stream and overlap the dgrad chain.
    def wgrad_stream(self, device):
        st = self._wg_stream.get(device)
        if st is None:
            # A NON-default priority, for the hardware queue it brings rather than for the scheduling: the HIP runtime multiplexes
            # all streams of one priority over a small pool of hardware queues, and once other streams exist (RCCL creates
            # several at communicator init) a default-priority side stream lands on the MAIN stream's queue -- the weight
            # gradients then run strictly between the main stream's kernels (measured: zero overlap, 87.7 -> 78.5 volumes/s
            # with nothing but a one-rank process group alive).  Each priority has its own queue pool.  "low" is also the
            # right scheduling hint: the data-gradient chain on the main stream is the critical path.
            st = _priority_stream(device, "low")
            self._wg_stream[device] = st
        return st

    def join_wgrad_stream(self):
        for st in self._wg_stream.values():
            torch.cuda.current_stream(st.device).wait_stream(st)
        self._wg_keep.clear()                  # (blocks freed now are reused in main-stream order, which follows the side stream)

    @contextlib.contextmanager
    def _on_side_stream(self, device, *operands):
        """The hand-off to the weight-gradient side stream: it waits for the current stream, the launches of the body go to it, and on
        a normal exit every operand given (None: skipped) is recorded on it, so that its block is not reused before the side stream
        has passed this point.  Also under hipGraph capture: the side stream joins the capture through wait_stream and becomes a
        parallel branch of the graph; record_stream defers the operands' blocks until the capture ends (no reuse inside the graph)."""
        side = self.wgrad_stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            yield
        for t in operands:
            if t is not None:
                t.record_stream(side)

    def wgrad(self, op, x, in_scale, in_shift, slope, dy, cout, inv_map, has_bias_map, w_numel, w_ref_shape=None, prec=None, allow_async=False):
        if self.wgrad_async and allow_async:
            with self._on_side_stream(x.device, x, dy, in_scale, in_shift):
                return self._wgrad_impl(op, x, in_scale, in_shift, slope, dy, cout, inv_map, has_bias_map, w_numel, w_ref_shape, prec)
        return self._wgrad_impl(op, x, in_scale, in_shift, slope, dy, cout, inv_map, has_bias_map, w_numel, w_ref_shape, prec)

    # Gradient-sink form (cwf.optim.GradSink, used by the Trainer): the layer's split-K slabs go to a buffer of its own and the
    # reduction of ALL layers of a backward phase is one launch (wgrad_flush) that writes dW / db straight into the flat gradient
    # buffer -- no per-layer reduce launch, no per-layer gradient tensors, no concatenation before the optimizer.
    def wgrad_release(self):
        """Enqueue the weight-gradient launches held back since `wgrad_defer` was set (see Trainer._fwd_bwd: the decoder's
        full-resolution weight gradients wait until backward reaches the GPU-light middle of the model, where they fill idle CUs
        instead of competing with the decoder's own HBM-bound data gradients)."""
        self.wgrad_defer = False
        held, self._wg_held = self._wg_held, []
        if not held:
            return
        if not self.wgrad_async:
            for args in held:
                self.wgrad_to(*args, allow_async=True)
            return
        # ONE hand-over to the side stream for the whole batch (instead of an event + stream switch + four record_stream calls per
        # launch); the operands stay referenced until the side stream is joined (join_wgrad_stream) instead of being recorded on it
        with self._on_side_stream(held[0][2].device):
            for args in held:
                self._wgrad_to_impl(*args)
        self._wg_keep.extend(held)

    def channel_sum_to(self, dy, out, allow_async=False):
        """out[c] = sum over (n, voxels) of dy[..., c] (the bias gradient of a layer whose slabs carry no bias row): a full pass over
        dy that only the optimizer waits for -- on the weight-gradient side stream when that is in use."""
        if self.wgrad_async and allow_async:
            with self._on_side_stream(dy.device, dy):
                self.stats_channel_sum(self.in_stats(dy), out)
        else:
            self.stats_channel_sum(self.in_stats(dy), out)
            self._wg_sync_needed = self.wgrad_async

    def dy_scale_ok(self, op, cin, cout, nvox):
        """wgrad_to(..., dy_scale=) is implemented for this layer (the full-resolution kernel of the <= 16 -> 16 layers, bf16 modes)"""
        return op == pk.CONV3_S1 and cin <= 16 and cout == 16 and nvox >= 32768 and (_WGRAD_PRECISION or _PRECISION) != "fp32" and \
            not self.bf16_operands_ok(op, cin, cout, nvox)

    def wgrad_to(self, key, op, x, in_scale, in_shift, slope, dy, cout, inv_map, dw_dst, db_dst, prec=None, x16=None, dy16=None, dy_scale=None,
                 allow_async=False):
        """x16 / dy16: bf16 operand images (see bf16_operands_ok).  Given one of them for an eligible layer, the other is made by a
        conversion pass in front of the launch (on the stream the launch runs on); x / dy are then not read.
        dy_scale: [N, cout] fp32, dy is taken as dy * dy_scale[n, c] (see dy_scale_ok); refused where no kernel of this call applies it."""
        if dy_scale is not None:
            self._check_dy_scale(op, x, dy, cout, prec, dy_scale)
        if self.wgrad_async and allow_async and self.wgrad_defer:
            self._wg_held.append((key, op, x, in_scale, in_shift, slope, dy, cout, inv_map, dw_dst, db_dst, prec, x16, dy16, dy_scale))
            return
        if self.wgrad_async and allow_async:
            with self._on_side_stream(x.device, x, dy, in_scale, in_shift, x16, dy16, dy_scale):
                self._wgrad_to_impl(key, op, x, in_scale, in_shift, slope, dy, cout, inv_map, dw_dst, db_dst, prec, x16, dy16, dy_scale)
        else:
            self._wgrad_to_impl(key, op, x, in_scale, in_shift, slope, dy, cout, inv_map, dw_dst, db_dst, prec, x16, dy16, dy_scale)
            self._wg_sync_needed = self.wgrad_async          # a main-stream producer: the side-stream reduce must wait for it
        if len(self._wg_pending) >= self.flush_every:
            # reduce in instalments: the LAST reduce of backward (after the stem's weight gradient) is exposed before the optimizer
            # step -- it should carry a handful of layers, not a whole phase.  (The Trainer switches this off in hipGraph mode:
            # the descriptor tables are keyed by their rows and must already exist when the capture runs.)
            self.wgrad_flush(x.device)

    def _check_dy_scale(self, op, x, dy, cout, prec, dy_scale):
        # only the fp32-tensor kernel of dy_scale_ok's layers scales dy while staging it: the bf16-image kernels and the fp32 mode would
        # drop the scale (or run in another precision), so such a call is an error, never a different computation
        n, do, ho, wo = dy.shape[0], dy.shape[1], dy.shape[2], dy.shape[3]
        mode = prec or _WGRAD_PRECISION or _PRECISION
        if mode == "fp32" or not self.dy_scale_ok(op, x.shape[-1], cout, do * ho * wo):
            raise _lib.CwfError("wgrad_to(dy_scale=) is not implemented for this layer / mode (op %d, %d -> %d channels, %d voxels, %s)"
                                % (op, x.shape[-1], cout, do * ho * wo, mode))
        if (tuple(dy_scale.shape) != (n, cout) or dy_scale.dtype != _f32 or not dy_scale.is_contiguous() or dy_scale.device != dy.device
                or dy_scale.data_ptr() % 16):
            raise _lib.CwfError("dy_scale must be a contiguous, 16-byte aligned float32 [%d, %d] tensor on %s" % (n, cout, dy.device))

    def _wgrad_to_impl(self, key, op, x, in_scale, in_shift, slope, dy, cout, inv_map, dw_dst, db_dst, prec, x16=None, dy16=None, dy_scale=None):
        x, x_ldc = cl(x)
        dy, dy_ldc = cl(dy)
        n, di, hi, wi, cin = x.shape
        _, do, ho, wo, _ = dy.shape
        # eligible layers always take the bf16-image kernel; an image nobody handed over is made here, i.e. on the stream this launch
        # runs on (normally the side stream, which has slack: the main stream's kernels are the step's critical path)
        use16 = self.bf16_operands_ok(op, cin, cout, do * ho * wo) if prec is None else 0
        nsplit, slab = self._wgrad_plan(op, dy.shape, cin, cout, (inv_map,))
        part = self._wgrad_slabs(key, x.device, nsplit * slab)
        a = self._wgrad_args(op, x, x_ldc, in_scale, in_shift, slope, dy, dy_ldc, cout, part, prec)
        if use16:
            if x16 is None:
                x16 = self.to_bf16(x, in_scale, in_shift, slope)
            if dy16 is None:
                dy16 = self.to_bf16(dy)
            assert x16.dtype == torch.bfloat16 and dy16.dtype == torch.bfloat16 and x16.is_contiguous() and dy16.is_contiguous()
            assert tuple(x16.shape) == (n, di, hi, wi, cin) and tuple(dy16.shape) == (n, do, ho, wo, cout)
            a.xa16, a.dy16, a.zero16 = x16.data_ptr(), dy16.data_ptr(), self.zero16(x.device).data_ptr()
        a.dy_scale = _p(dy_scale)
        used = ctypes.c_int(0)
        self._call("cwf_wgrad", ctypes.addressof(a), ctypes.addressof(used), self._stream())
        self._wg_pending.append((part.data_ptr(), inv_map.data_ptr(), dw_dst.data_ptr(), _p(db_dst), int(slab), int(used.value)))

    def _wgrad_plan(self, op, dy_shape, cin, cout, inv_maps):
        """(nsplit, slab): the library's split-K plan of a layer with output gradient [n, do, ho, wo, .] -- at most nsplit slabs of
        `slab` floats -- checked against the layer's (the group's layers') inverse maps"""
        n, do, ho, wo = dy_shape[:4]
        nsplit = self.lib.cwf_wgrad_nsplit(op, n, do, ho, wo, cin, cout)
        slab = self.lib.cwf_wgrad_slab_floats(op, cin, cout)
        if nsplit <= 0 or slab <= 0 or any(slab != m.numel() for m in inv_maps):
            raise _lib.CwfError("cwf_wgrad plan failed (%d, %d, %s)" % (nsplit, slab, [m.numel() for m in inv_maps]))
        return nsplit, slab

    def _wgrad_slabs(self, key, device, nfloats):
        """the slab buffer of layer `key` on `device`: persistent, also across graph capture, so the descriptor tables of wgrad_flush
        stay valid"""
        part = self._wg_part.get((key, device))
        if part is None or part.numel() < nfloats:
            part = self._wg_part[(key, device)] = torch.empty(int(nfloats), dtype=_f32, device=device)
        return part

    @staticmethod
    def _wgrad_args(op, x, x_ldc, in_scale, in_shift, slope, dy, dy_ldc, cout, part, prec):
        """struct cwf_wgrad_args of one layer (x / dy channels-last views, part its slab buffer)"""
        n, di, hi, wi, cin = x.shape
        _, do, ho, wo, _ = dy.shape
        return _lib.WgradArgs(op=op, precision=_lib.PRECISION[prec or _WGRAD_PRECISION or _PRECISION], x=x.data_ptr(), x_ldc=x_ldc,
                              in_scale=_p(in_scale), in_shift=_p(in_shift), in_slope=float(slope), dy=dy.data_ptr(), dy_ldc=dy_ldc,
                              partial=part.data_ptr(), N=n, Di=di, Hi=hi, Wi=wi, Cin=cin, Do=do, Ho=ho, Wo=wo, Cout=cout)

    def wgrad_to_grouped(self, keys, op, xs, dys, cout, inv_maps, dw_dsts, db_dsts, prec=None, allow_async=False):
        """wgrad_to for G same-shape 3x3x3 stride-1 layers without prologue (channel-group views xs[q] / dys[q] of shared buffers):
        ONE slab launch (cwf_wgrad with groups); each layer keeps its own slab buffer and row in the batched reduce."""
        mode = prec or _WGRAD_PRECISION or _PRECISION
        if mode == "fp32" or (self.wgrad_async and allow_async and self.wgrad_defer):
            for q in range(len(keys)):
                self.wgrad_to(keys[q], op, xs[q], None, None, 1.0, dys[q], cout, inv_maps[q], dw_dsts[q], db_dsts[q], prec=prec, allow_async=allow_async)
            return
        if self.wgrad_async and allow_async:
            with self._on_side_stream(xs[0].device, *xs, *dys):
                self._wgrad_to_grouped_impl(keys, op, xs, dys, cout, inv_maps, dw_dsts, db_dsts, mode)
        else:
            self._wgrad_to_grouped_impl(keys, op, xs, dys, cout, inv_maps, dw_dsts, db_dsts, mode)
            self._wg_sync_needed = self.wgrad_async

    def _wgrad_to_grouped_impl(self, keys, op, xs, dys, cout, inv_maps, dw_dsts, db_dsts, mode):
        G = len(keys)
        x0, x_ldc = cl(xs[0])
        d0, dy_ldc = cl(dys[0])
        if any(cl(t)[0].data_ptr() != t.data_ptr() for t in list(xs) + list(dys)):
            # the launch takes every group's own pointer with ONE row pitch: a view that cl() has to copy cannot be sent
            raise _lib.CwfError("wgrad_to_grouped needs group views the kernels can read in place (channels-last, 16-byte aligned "
                                "starts, a row pitch that is a multiple of 4)")
        n, di, hi, wi, cin = x0.shape
        _, do, ho, wo, _ = d0.shape
        nsplit, slab = self._wgrad_plan(op, d0.shape, cin, cout, inv_maps)
        parts = []
        for q in range(G):
            assert xs[q].stride() == xs[0].stride() and dys[q].stride() == dys[0].stride() and xs[q].shape == xs[0].shape
            parts.append(self._wgrad_slabs(keys[q], x0.device, nsplit * slab))
        a = _lib.WgradArgs(op=op, precision=_lib.PRECISION[mode], x_ldc=x_ldc, in_slope=1.0, dy_ldc=dy_ldc, groups=G,
                           N=n, Di=di, Hi=hi, Wi=wi, Cin=cin, Do=do, Ho=ho, Wo=wo, Cout=cout)
        for q in range(G):
            a.x_g[q], a.dy_g[q], a.partial_g[q] = xs[q].data_ptr(), dys[q].data_ptr(), parts[q].data_ptr()
        used = ctypes.c_int(0)
        self._call("cwf_wgrad", ctypes.addressof(a), ctypes.addressof(used), self._stream())
        for q in range(G):
            self._wg_pending.append((parts[q].data_ptr(), inv_maps[q].data_ptr(), dw_dsts[q].data_ptr(), _p(db_dsts[q]), int(slab), int(used.value)))

    def wgrad_flush(self, device=None):
        """One batched reduce for every layer queued by wgrad_to since the last flush (on the weight-gradient side stream when
        that is in use: it follows the queued kernels in stream order)."""
        rows = self._wg_pending
        if not rows:
            return
        self._wg_pending = []
        device = device or torch.device("cuda", _current_device())
        key = (device, tuple(rows))
        table = self._wg_tables.get(key)
        if table is None:                       # static across steps (persistent buffers, static shapes): built once
            import struct
            raw = b"".join(struct.pack("<QQQQqii", r[0], r[1], r[2], r[3], r[4], r[5], 0) for r in rows)
            host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
            if torch.cuda.is_current_stream_capturing():
                # (only if no eager step preceded the capture) a pinned source keeps the copy capturable; it must outlive the graph
                host = host.pin_memory()
                self._wg_tables[("pinned",) + key] = host
                table = torch.empty_like(host, device=device)
                table.copy_(host, non_blocking=True)
            else:
                table = host.to(device)
            self._wg_tables[key] = table
        if self.wgrad_async:
            side = self.wgrad_stream(device)
            if self._wg_sync_needed:
                side.wait_stream(torch.cuda.current_stream(device))
                self._wg_sync_needed = False
            with torch.cuda.stream(side):
                self._call("cwf_wgrad_reduce_batched", table.data_ptr(), len(rows), self._stream())
        else:
            self._call("cwf_wgrad_reduce_batched", table.data_ptr(), len(rows), self._stream())

    def _wgrad_impl(self, op, x, in_scale, in_shift, slope, dy, cout, inv_map, has_bias_map, w_numel, w_ref_shape=None, prec=None):
        """returns (dW flat [w_numel], db [cout] or None)"""
        x, x_ldc = cl(x)
        dy, dy_ldc = cl(dy)
        nsplit, slab = self._wgrad_plan(op, dy.shape, x.shape[4], cout, (inv_map,))
        part = self.workspace("wgrad", nsplit * slab, x.device)
        a = self._wgrad_args(op, x, x_ldc, in_scale, in_shift, slope, dy, dy_ldc, cout, part, prec)
        used = ctypes.c_int(0)
        self._call("cwf_wgrad", ctypes.addressof(a), ctypes.addressof(used), self._stream())
        nsplit = used.value
        dw = torch.empty(w_numel, dtype=_f32, device=x.device)
        db = torch.empty(cout, dtype=_f32, device=x.device) if has_bias_map else None
        self._call("cwf_wgrad_reduce", part.data_ptr(), nsplit, slab, inv_map.data_ptr(), dw.data_ptr(), _p(db), self._stream())
        return dw, db

    def gather_batched(self, table, nlayers, max_n, split_bf16=False):
        self._call("cwf_gather_split_bf16" if split_bf16 else "cwf_gather_batched", table.data_ptr(), nlayers, max_n, self._stream())

    # ------------------------------------------------------------------ K3
    def new_stats(self, n, c, device):
        return self._zeros_f64((n, c, 2), device)

    def in_finalize(self, stats, nvox, eps=1e-5):
        n, c, _ = stats.shape
        scale = torch.empty((n, c), dtype=_f32, device=stats.device)
        shift = torch.empty((n, c), dtype=_f32, device=stats.device)
        self._call("cwf_in_finalize", stats.data_ptr(), scale.data_ptr(), shift.data_ptr(), n * c, nvox, eps, self._stream())
        return scale, shift

    def in_stats(self, x):
        x, ldc = cl(x)
        n, d, h, w, c = x.shape
        stats = self.new_stats(n, c, x.device)
        self._call("cwf_in_stats", x.data_ptr(), ldc, stats.data_ptr(), n, d * h * w, c, self._stream())
        return stats

    def norm_act_add(self, x, scale, shift, slope, residual=None, want16=False):
        """want16: also returns bf16(y) (the operand image of a consuming layer's weight gradient): (y, y16)"""
        x, ldc = cl(x)
        n, d, h, w, c = x.shape
        y = torch.empty((n, d, h, w, c), dtype=_f32, device=x.device)
        y16 = torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=x.device) if want16 else None
        r_ldc = 0
        if residual is not None:
            residual, r_ldc = cl(residual)
        self._call("cwf_norm_act_add_ex", x.data_ptr(), ldc, scale.data_ptr(), shift.data_ptr(), float(slope), _p(residual), r_ldc,
                   y.data_ptr(), c, _p(y16), n, d * h * w, c, self._stream())
        return (y, y16) if want16 else y

    def in_bwd(self, dy, x, scale, shift, slope, dx_add=None):
        """dx for y = act(IN(x)) given dy = dL/dy (full InstanceNorm backward, statistics included)."""
        dy, dy_ldc = cl(dy)
        x, x_ldc = cl(x)
        n, d, h, w, c = x.shape
        v = d * h * w
        sums = self.new_stats(n, c, x.device)
        self._call("cwf_in_bwd_stats", dy.data_ptr(), dy_ldc, x.data_ptr(), x_ldc, scale.data_ptr(), shift.data_ptr(), float(slope),
                   sums.data_ptr(), n, v, c, self._stream())
        dx = torch.empty((n, d, h, w, c), dtype=_f32, device=x.device)
        a_ldc = 0
        if dx_add is not None:
            dx_add, a_ldc = cl(dx_add)
        self._call("cwf_in_bwd_apply", dy.data_ptr(), dy_ldc, x.data_ptr(), x_ldc, scale.data_ptr(), shift.data_ptr(), float(slope),
                   sums.data_ptr(), _p(dx_add), a_ldc, dx.data_ptr(), c, n, v, c, self._stream())
        return dx

    # ------------------------------------------------------------------ K6/K7
    def gemm(self, a, sa, b, sb, c, sc, m, n, k, zb=1, zh=1, bias=None, residual=None, sr=(0, 0, 0), alpha=1.0, act=0,
             accumulate=False, a_off=0, b_off=0, c_off=0, r_off=0):
        """sa = (m, k, zb, zh) element strides of A; sb = (k, n, zb, zh); sc = (m, zb, zh); offsets in elements."""
        self._call("cwf_gemm", a.data_ptr() + 4 * a_off, sa[0], sa[1], sa[2], sa[3],
                   b.data_ptr() + 4 * b_off, sb[0], sb[1], sb[2], sb[3],
                   c.data_ptr() + 4 * c_off, sc[0], sc[1], sc[2],
                   _p(bias), (residual.data_ptr() + 4 * r_off) if residual is not None else 0, sr[0], sr[1], sr[2],
                   m, n, k, zb, zh, float(alpha), act, int(accumulate), self._stream())
        return c

    def layernorm_fwd(self, x, gamma, beta, eps=1e-5):
        rows, e = x.numel() // x.shape[-1], x.shape[-1]
        x = x.contiguous()
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=_f32, device=x.device)
        rstd = torch.empty(rows, dtype=_f32, device=x.device)
        self._call("cwf_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                   rows, e, eps, self._stream())
        return y, mean, rstd

    def layernorm_bwd(self, dy, x, gamma, mean, rstd, dgamma, dbeta):
        rows, e = x.numel() // x.shape[-1], x.shape[-1]
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        self._call("cwf_layernorm_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                   dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, e, 0, self._stream())
        return dx

    def softmax_rows_(self, s):
        cols = s.shape[-1]
        self._call("cwf_softmax_rows", s.data_ptr(), s.numel() // cols, cols, cols, self._stream())
        return s

    def softmax_rows_bwd_(self, p, dp):
        cols = p.shape[-1]
        self._call("cwf_softmax_rows_bwd", p.data_ptr(), dp.data_ptr(), p.numel() // cols, cols, cols, self._stream())
        return dp

    def gelu_bwd(self, x, dy):
        dx = torch.empty_like(x)
        self._call("cwf_gelu_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), self._stream())
        return dx

    def colsum(self, x2d):
        rows, cols = x2d.shape
        out = torch.empty(cols, dtype=_f32, device=x2d.device)
        self._call("cwf_colsum", x2d.data_ptr(), rows, cols, x2d.stride(0), out.data_ptr(), 0, self._stream())
        return out

    # ------------------------------------------------------------------ K4/K5
    def window_to_tokens(self, x, patch):
        x, ldc = cl(x)
        b, d, h, w, c = x.shape
        p0, p1, p2 = patch
        tok = torch.empty((b, (d // p0) * (h // p1) * (w // p2), c * p0 * p1 * p2), dtype=_f32, device=x.device)
        self._call("cwf_window_to_tokens", x.data_ptr(), ldc, tok.data_ptr(), b, d, h, w, c, p0, p1, p2, self._stream())
        return tok

    def tokens_to_window(self, tok, size, channels, patch):
        b = tok.shape[0]
        d, h, w = size
        p0, p1, p2 = patch
        tok = tok.contiguous()
        x = torch.empty((b, d, h, w, channels), dtype=_f32, device=tok.device)
        self._call("cwf_tokens_to_window", tok.data_ptr(), x.data_ptr(), channels, b, d, h, w, channels, p0, p1, p2, 0, self._stream())
        return x

    def window_to_tokens_g(self, x, groups, patch):
        """x [B,D,H,W,groups*C] -> tok [groups,B,T,C*p0*p1*p2] (one launch for the three sub-regions)"""
        x, ldc = cl(x)
        b, d, h, w, ct = x.shape
        c = ct // groups
        p0, p1, p2 = patch
        tok = torch.empty((groups, b, (d // p0) * (h // p1) * (w // p2), c * p0 * p1 * p2), dtype=_f32, device=x.device)
        self._call("cwf_window_to_tokens_g", x.data_ptr(), ldc, tok.data_ptr(), groups, b, d, h, w, c, p0, p1, p2, self._stream())
        return tok

    def tokens_to_window_g(self, tok, size, channels, patch):
        """tok [groups,B,T,E] -> x [B,D,H,W,groups*channels]"""
        g, b = tok.shape[0], tok.shape[1]
        d, h, w = size
        p0, p1, p2 = patch
        tok = tok.contiguous()
        x = torch.empty((b, d, h, w, g * channels), dtype=_f32, device=tok.device)
        self._call("cwf_tokens_to_window_g", tok.data_ptr(), x.data_ptr(), g * channels, g, b, d, h, w, channels, p0, p1, p2, self._stream())
        return x

    def cat3_channels(self, parts, shape, device):
        """[N,D,H,W,C] x 3 (None = zeros) -> [N,D,H,W,3C]"""
        n, d, h, w, c = shape
        parts = [None if t is None else t.contiguous() for t in parts]
        y = torch.empty((n, d, h, w, 3 * c), dtype=_f32, device=device)
        self._call("cwf_cat3_channels", _p(parts[0]), _p(parts[1]), _p(parts[2]), y.data_ptr(), n * d * h * w, c, self._stream())
        return y

    def token_scores(self, feats, query):
        """feats [B,T,E]; query [1,1,E] (shared) or [B,1,E]."""
        b, t, e = feats.shape
        score = torch.empty((b, t), dtype=_f32, device=feats.device)
        qbs = 0 if query.shape[0] == 1 else e
        self._call("cwf_token_scores", feats.data_ptr(), query.data_ptr(), qbs, score.data_ptr(), b, t, e, self._stream())
        return score

    def topk(self, score, k):
        b, t = score.shape
        idx = torch.empty((b, k), dtype=torch.int32, device=score.device)
        self._call("cwf_topk", score.data_ptr(), idx.data_ptr(), b, t, k, self._stream())
        return idx

    def gather_tokens(self, feats, index, head, keep=None, pe_odd=1.0):
        b, t, e = feats.shape
        k = index.shape[1]
        seq = torch.empty((b, k + 1, e), dtype=_f32, device=feats.device)
        hbs = 0 if head.shape[0] == 1 else e
        self._call("cwf_gather_tokens", feats.data_ptr(), index.data_ptr(), head.data_ptr(), hbs, _p(keep), float(pe_odd),
                   seq.data_ptr(), b, t, k, e, self._stream())
        return seq

    def gather_tokens_bwd(self, dseq, index, keep, dfeats, dhead):
        """dfeats [B,T,E] accumulated in place (may be None); dhead [1 or B,1,E] accumulated in place (may be None)."""
        b, k1, e = dseq.shape
        dseq = dseq.contiguous()
        t = dfeats.shape[1] if dfeats is not None else 0
        dhbs = 0 if (dhead is None or dhead.shape[0] == 1) else e
        self._call("cwf_gather_tokens_bwd", dseq.data_ptr(), index.data_ptr(), _p(keep), _p(dfeats), _p(dhead), dhbs,
                   b, t, k1 - 1, e, self._stream())

    def scatter_rows(self, feats, index, rows, gate=None):
        """rows: [B,k,E] view (row stride / batch stride taken from the tensor); gate [B,1,E] view or None."""
        b, t, e = feats.shape
        k = index.shape[1]
        assert rows.stride(2) == 1
        out = torch.empty((b, t, e), dtype=_f32, device=feats.device)
        gbs = gate.stride(0) if gate is not None else 0
        self._call("cwf_scatter_rows", feats.data_ptr(), index.data_ptr(), rows.data_ptr(), rows.stride(1), rows.stride(0),
                   _p(gate), gbs, out.data_ptr(), b, t, k, e, self._stream())
        return out

    def scatter_rows_bwd(self, dout, index, scat, gate, k, need_feats=True, need_rows=True):
        """returns (dfeats [B,T,E] or None, drows [B,k,E] or None, dgate [B,1,E] or None)"""
        b, t, e = dout.shape
        dout = dout.contiguous()
        dfeats = torch.empty((b, t, e), dtype=_f32, device=dout.device) if need_feats else None
        drows = torch.empty((b, k, e), dtype=_f32, device=dout.device) if need_rows else None
        dgate = torch.zeros((b, 1, e), dtype=_f32, device=dout.device) if gate is not None else None
        gbs = gate.stride(0) if gate is not None else 0
        self._call("cwf_scatter_rows_bwd", dout.data_ptr(), index.data_ptr(), _p(scat), _p(gate), gbs,
                   _p(dfeats), 0, _p(drows), e, k * e, _p(dgate), e, b, t, k, e, self._stream())
        return dfeats, drows, dgate

    # ------------------------------------------------------------------ K6/K7, round-2 fused forms (one coupler block = 4 launches)
    def _gemm_ex(self, **kw):
        g = _lib.GemmArgs()
        for k, v in kw.items():
            setattr(g, k, v)
        self._call("cwf_gemm_ex", ctypes.addressof(g), self._stream())

    def _drop_kw(self, prefix, drop, numel, dev):
        if not drop:
            return {}
        off, p, p2 = drop
        return {prefix + "_off": off, prefix + "_n": numel, prefix + "_p": float(p), prefix + "_p2": float(p2), "rng": self.rng(dev).data_ptr()}

    def linear_fwd(self, x, w, bias, out, x2=None, split_n=0, act=0, pre=None, drop=None, residual=None):
        """out = drop(act(x' w^T + bias)) + residual ; x' = x for output columns < split_n, x2 beyond (2-D row-major views)."""
        m, k = x.shape
        grouped = isinstance(w, (list, tuple))          # G weight sets: rows of x / out are G stacked problems (z = group)
        G = len(w) if grouped else 1
        w0 = w[0] if grouped else w
        n = w0.shape[0]
        assert x.stride(1) == 1 and w0.stride(1) == 1 and out.stride(1) == 1 and out.shape == (m, n) and m % G == 0
        mg = m // G
        kw = dict(A=x.data_ptr(), sa_m=x.stride(0), sa_k=1, sa_zb=mg * x.stride(0), B=w0.data_ptr(), sb_k=1, sb_n=w0.stride(0),
                  C=out.data_ptr(), sc_m=out.stride(0), sc_zb=mg * out.stride(0), bias=_p(bias) if not grouped else 0,
                  M=mg, N=n, K=k, ZB=G, ZH=1, alpha=1.0, act=act)
        if grouped:
            assert all(t.stride() == w0.stride() for t in w)
            kw["B_tab"] = _tab(w)
            if bias is not None:
                kw["bias_tab"] = _tab(bias)
        if x2 is not None:
            assert x2.stride() == x.stride() and x2.shape == x.shape
            kw.update(A2=x2.data_ptr(), split_n=split_n)
        if pre is not None:
            assert pre.stride() == out.stride()
            kw["C2"] = pre.data_ptr()
        if residual is not None:
            assert residual.stride(1) == 1
            kw.update(residual=residual.data_ptr(), sr_m=residual.stride(0), sr_zb=mg * residual.stride(0))
        kw.update(self._drop_kw("c_drop", drop, m * n, x.device))
        if drop:
            assert out.stride(0) == n           # the mask index is the element offset inside out
        self._gemm_ex(**kw)
        return out

    def linear_dgrad(self, dy, w, drop=None, out=None):
        """dx = (dy * keep) w ; dy [M,N] (row stride from the view), w [N,K] view."""
        m, n = dy.shape
        grouped = isinstance(w, (list, tuple))
        G = len(w) if grouped else 1
        w0 = w[0] if grouped else w
        k = w0.shape[1]
        assert dy.stride(1) == 1 and w0.stride(1) == 1 and m % G == 0
        mg = m // G
        dx = out if out is not None else torch.empty((m, k), dtype=_f32, device=dy.device)
        kw = dict(A=dy.data_ptr(), sa_m=dy.stride(0), sa_k=1, sa_zb=mg * dy.stride(0), B=w0.data_ptr(), sb_k=w0.stride(0), sb_n=1,
                  C=dx.data_ptr(), sc_m=dx.stride(0), sc_zb=mg * dx.stride(0), M=mg, N=k, K=n, ZB=G, ZH=1, alpha=1.0)
        if grouped:
            assert all(t.stride() == w0.stride() for t in w)
            kw["B_tab"] = _tab(w)
        kw.update(self._drop_kw("a_drop", drop, m * n, dy.device))
        if drop:
            assert dy.stride(0) == n
        self._gemm_ex(**kw)
        return dx

    def linear_wgrad(self, dy, x, dw, dbias=None, x2=None, split_m=0, accumulate=False, drop=None):
        """dw (+)= (dy * keep)^T x' ; dbias (+)= column sums of dy * keep ; x' = x for dw rows < split_m, x2 beyond."""
        m, n = dy.shape
        k = x.shape[1]
        grouped = isinstance(dw, (list, tuple))
        G = len(dw) if grouped else 1
        dw0 = dw[0] if grouped else dw
        assert dy.stride(1) == 1 and x.stride(1) == 1 and dw0.shape == (n, k) and dw0.is_contiguous() and m % G == 0
        mg = m // G
        kw = dict(A=dy.data_ptr(), sa_m=1, sa_k=dy.stride(0), sa_zb=mg * dy.stride(0), B=x.data_ptr(), sb_k=x.stride(0), sb_n=1,
                  sb_zb=mg * x.stride(0), C=dw0.data_ptr(), sc_m=k, M=n, N=k, K=mg, ZB=G, ZH=1, alpha=1.0, accumulate=int(accumulate))
        if grouped:
            assert all(t.shape == dw0.shape and t.is_contiguous() for t in dw)
            kw["C_tab"] = _tab(dw)
        if x2 is not None:
            assert x2.stride() == x.stride()
            kw.update(B2=x2.data_ptr(), split_m=split_m)
        if dbias is not None:
            if grouped:
                kw.update(rowsum_tab=_tab(dbias), rowsum_acc=int(accumulate))
            else:
                kw.update(rowsum=dbias.data_ptr(), rowsum_acc=int(accumulate))
        kw.update(self._drop_kw("a_drop", drop, m * n, dy.device))
        if drop:
            assert dy.stride(0) == n
        self._gemm_ex(**kw)

    def ln_pair_fwd(self, x, x2, perm_T, g1, b1, g2, b2, eps=1e-5):
        """g1 ... b2: tensors, or lists of G tensors (rows = G stacked problems, one LayerNorm parameter set each)"""
        rows, e = x.shape
        ya = torch.empty_like(x)
        yb = torch.empty_like(x) if x2 is not None else None
        stats = torch.empty((2 if x2 is not None else 1, rows, 2), dtype=_f32, device=x.device)
        P, G = _ln_params(g1=g1, b1=b1, g2=g2, b2=b2)
        self._call("cwf_ln_pair_fwd_g", x.data_ptr(), _p(x2), perm_T, ctypes.addressof(P), G, ya.data_ptr(), _p(yb),
                   stats.data_ptr(), rows, e, eps, self._stream())
        return ya, yb, stats

    def ln_pair_bwd(self, dy, da, db, x, x2, perm_T, g1, g2, stats, dg1, db1, dg2, db2, accumulate, want_dx2):
        rows, e = x.shape
        dx = torch.empty_like(x)
        dx2 = torch.empty_like(x) if want_dx2 else None
        P, G = _ln_params(g1=g1, g2=g2, dg1=dg1, db1=db1, dg2=dg2, db2=db2)
        self._call("cwf_ln_pair_bwd_g", _p(dy), da.data_ptr(), _p(db), x.data_ptr(), _p(x2), perm_T, ctypes.addressof(P), G, stats.data_ptr(),
                   dx.data_ptr(), _p(dx2), rows, e, int(accumulate), self._stream())
        return dx, dx2

    def attn_fwd(self, qkv, z, t, heads, drop=None):
        e = qkv.shape[1] // 3
        o = torch.empty((z * t, e), dtype=_f32, device=qkv.device)
        off, p = (drop[0], drop[1]) if drop else (0, 0.0)
        self._call("cwf_attn_fwd", qkv.data_ptr(), qkv.stride(0), o.data_ptr(), e, z, t, e, heads, float((e // heads) ** -0.5),
                   self.rng(qkv.device).data_ptr(), off, float(p), self._stream())
        return o

    def attn_bwd(self, qkv, d_o, z, t, heads, drop=None):
        e = qkv.shape[1] // 3
        assert d_o.is_contiguous()
        dqkv = torch.empty_like(qkv)
        off, p = (drop[0], drop[1]) if drop else (0, 0.0)
        # the probabilities between the two launches: a persistent buffer, so the launch plan and a captured graph see one pointer
        nbytes = int(self.lib.cwf_attn_bwd_ws_bytes(z, t, heads))
        ws = self.workspace("attn_bwd", nbytes // 4, qkv.device)
        self._call("cwf_attn_bwd_ws", qkv.data_ptr(), qkv.stride(0), d_o.data_ptr(), e, dqkv.data_ptr(), z, t, e, heads,
                   float((e // heads) ** -0.5), self.rng(qkv.device).data_ptr(), off, float(p), ws.data_ptr(), ws.numel() * 4, self._stream())
        return dqkv

    def gelu_bwd_drop(self, z, dh, drop=None):
        dz = torch.empty_like(z)
        off, p = (drop[0], drop[1]) if drop else (0, 0.0)
        self._call("cwf_gelu_bwd_drop", z.data_ptr(), dh.data_ptr(), dz.data_ptr(), z.numel(), self.rng(z.device).data_ptr(), off, float(p), self._stream())
        return dz

    # ------------------------------------------------------------------ K4/K5, round-2 forms
    def token_scores2(self, feats, q1, q2=None):
        """q1 / q2: [1|B,1,E] tensors, or lists of G shared queries (sample b belongs to group b // (B/G))"""
        b, t, e = feats.shape
        s1 = torch.empty((b, t), dtype=_f32, device=feats.device)
        s2 = torch.empty((b, t), dtype=_f32, device=feats.device) if q2 is not None else None
        if isinstance(q1, (list, tuple)):
            G = len(q1)
            t1 = (ctypes.c_void_p * G)(*[q.data_ptr() for q in q1])
            t2 = (ctypes.c_void_p * G)(*[q.data_ptr() for q in q2]) if q2 is not None else None
            self._call("cwf_token_scores2_g", feats.data_ptr(), ctypes.addressof(t1), ctypes.addressof(t2) if t2 is not None else 0, G, b // G,
                       s1.data_ptr(), _p(s2), b, t, e, self._stream())
            return s1, s2
        self._call("cwf_token_scores2", feats.data_ptr(), q1.data_ptr(), 0 if q1.shape[0] == 1 else e, _p(q2),
                   0 if (q2 is None or q2.shape[0] == 1) else e, s1.data_ptr(), _p(s2), b, t, e, self._stream())
        return s1, s2

    def topk_inv(self, s0, s1, k):
        """-> (index0, inv0, index1, inv1); the second pair is None when s1 is None."""
        b, t = s0.shape
        i32 = torch.int32
        idx0 = torch.empty((b, k), dtype=i32, device=s0.device); inv0 = torch.empty((b, t), dtype=i32, device=s0.device)
        idx1 = inv1 = None
        if s1 is not None:
            idx1 = torch.empty((b, k), dtype=i32, device=s0.device); inv1 = torch.empty((b, t), dtype=i32, device=s0.device)
        self._call("cwf_topk_inv", s0.data_ptr(), idx0.data_ptr(), inv0.data_ptr(), _p(s1), _p(idx1), _p(inv1), b, t, k, self._stream())
        return idx0, inv0, idx1, inv1

    def index_inv(self, index, t):
        b, k = index.shape
        index = index.to(torch.int32).contiguous()
        inv = torch.empty((b, t), dtype=torch.int32, device=index.device)
        self._call("cwf_index_inv", index.data_ptr(), inv.data_ptr(), b, t, k, self._stream())
        return index, inv

    def gather_multi(self, jobs, k, e, p=0.0, pe_odd=1.0):
        """jobs: list of (feats [B,T,E], index [B,k], head [1|B,1,E], out view [B,k+1,E] with contiguous rows, drop_off)."""
        arr = (_lib.GatherJob * len(jobs))()
        b = jobs[0][0].shape[0]
        for i, (feats, index, head, out, off) in enumerate(jobs):
            assert out.stride(2) == 1 and out.stride(1) == e and feats.is_contiguous()
            if isinstance(head, (list, tuple)):              # one shared head per group of b // len(head) samples
                hg = (ctypes.c_void_p * 4)(*([h.data_ptr() for h in head] + [0] * (4 - len(head))))
                arr[i] = _lib.GatherJob(feats.data_ptr(), index.data_ptr(), 0, out.data_ptr(), 0, out.stride(0), feats.shape[1], off, hg, b // len(head))
            else:
                arr[i] = _lib.GatherJob(feats.data_ptr(), index.data_ptr(), head.data_ptr(), out.data_ptr(), 0 if head.shape[0] == 1 else e,
                                        out.stride(0), feats.shape[1], off, (ctypes.c_void_p * 4)(), 0)
        self._call("cwf_gather_multi", ctypes.addressof(arr), len(jobs), b, k, e, float(pe_odd), self.rng(jobs[0][0].device).data_ptr(), float(p), self._stream())

    def scatter_inv(self, feats, inv, rows, gate, want_gated=True, want_scat=False):
        """rows [B,k,E] / gate [B,1,E] views with unit inner stride -> (gated, scat)"""
        b, t, e = feats.shape
        gated = torch.empty_like(feats) if want_gated else None
        scat = torch.empty_like(feats) if want_scat else None
        self._call("cwf_scatter_inv", feats.data_ptr(), inv.data_ptr(), rows.data_ptr(), rows.stride(1), rows.stride(0), _p(gate),
                   gate.stride(0) if gate is not None else 0, _p(gated), _p(scat), b, t, e, self._stream())
        return gated, scat

    def scatter_bwd(self, dgated, dscat, feats, inv, index, rows, gate, dgate_extra, drows, dgate):
        """writes drows [B,k,E] view and dgate [B,1,E] view (both inside the coupler's output gradient)"""
        b, t, e = feats.shape
        k = index.shape[1]
        self._call("cwf_scatter_bwd", _p(dgated), _p(dscat), feats.data_ptr(), inv.data_ptr(), index.data_ptr(), rows.data_ptr(), rows.stride(1),
                   rows.stride(0), _p(gate), gate.stride(0) if gate is not None else 0, _p(dgate_extra),
                   dgate_extra.stride(0) if dgate_extra is not None else 0, drows.data_ptr(), drows.stride(1), drows.stride(0),
                   dgate.data_ptr(), dgate.stride(0), b, t, k, e, self._stream())

    def token_grad(self, dgated, dscat, gate, inv_p, inv_q, dseq_p, dseq_q, k, p=0.0, off_p=0, off_q=0):
        b, t = inv_p.shape
        e = dseq_p.shape[2]
        dfeats = torch.empty((b, t, e), dtype=_f32, device=dseq_p.device)
        self._call("cwf_token_grad", _p(dgated), _p(dscat), _p(gate), gate.stride(0) if gate is not None else 0, inv_p.data_ptr(), _p(inv_q),
                   dseq_p.data_ptr(), dseq_p.stride(0), _p(dseq_q), dseq_q.stride(0) if dseq_q is not None else 0,
                   self.rng(dseq_p.device).data_ptr(), off_p, off_q, float(p), dfeats.data_ptr(), b, t, k, e, self._stream())
        return dfeats

    def head_grad(self, a1, c1, a2, c2, out1=None, out2=None):
        """out1 = sum_b (a1[b] + c1[b]), out2 = sum_b (a2[b] + c2[b]); inputs are [B,E] row views with a common batch stride"""
        b, e = a1.shape
        bs = a1.stride(0)
        assert c1.stride(0) == bs and a2.stride(0) == bs and c2.stride(0) == bs
        if isinstance(out1, (list, tuple)):                  # G groups of b // G samples, one output pair per group
            G = len(out1)
            t1 = (ctypes.c_void_p * G)(*[t.data_ptr() for t in out1]); t2 = (ctypes.c_void_p * G)(*[t.data_ptr() for t in out2])
            self._call("cwf_head_grad_g", a1.data_ptr(), c1.data_ptr(), a2.data_ptr(), c2.data_ptr(), bs, ctypes.addressof(t1), ctypes.addressof(t2),
                       G, b // G, e, self._stream())
            return out1, out2
        o1 = out1 if out1 is not None else torch.empty((1, 1, e), dtype=_f32, device=a1.device)
        o2 = out2 if out2 is not None else torch.empty((1, 1, e), dtype=_f32, device=a1.device)
        self._call("cwf_head_grad", a1.data_ptr(), c1.data_ptr(), a2.data_ptr(), c2.data_ptr(), bs, o1.data_ptr(), o2.data_ptr(), b, e, self._stream())
        return o1, o2

    def sum_groups3(self, x):
        """x [3, ...] contiguous -> x[0] + x[1] + x[2]"""
        assert x.shape[0] == 3 and x.is_contiguous()
        y = torch.empty(x.shape[1:], dtype=_f32, device=x.device)
        n = y.numel()
        self._call("cwf_add3", x.data_ptr(), x.data_ptr() + 4 * n, x.data_ptr() + 8 * n, y.data_ptr(), n, self._stream())
        return y

    def bcast_groups3(self, d):
        """d [...] -> [3, ...] (three copies): the adjoint of sum_groups3 as ONE launch"""
        d = d.contiguous()
        y = torch.empty((3,) + tuple(d.shape), dtype=_f32, device=d.device)
        self._call("cwf_bcast3", d.data_ptr(), y.data_ptr(), d.numel(), self._stream())
        return y

    def stats_channel_sum(self, stats, out):
        """out[c] = sum_n stats[n][c][0]  (bias gradient of a transposed conv from the per-(n,c) sums of dy)"""
        n, c, _ = stats.shape
        self._call("cwf_stats_channel_sum", stats.data_ptr(), out.data_ptr(), n, c, self._stream())
        return out

    def add3(self, a, b, c):
        a, b, c = a.contiguous(), b.contiguous(), c.contiguous()
        y = torch.empty_like(a)
        self._call("cwf_add3", a.data_ptr(), b.data_ptr(), c.data_ptr(), y.data_ptr(), a.numel(), self._stream())
        return y

    # ------------------------------------------------------------------ K8/K10
    def upsample_softmax(self, logit, c, scale):
        """logit [N,d,h,w,>=c] (channel stride from the tensor) -> prob [N,d*s,h*s,w*s,c]"""
        n, d, h, w, _ = logit.shape
        prob = torch.empty((n, d * scale, h * scale, w * scale, c), dtype=_f32, device=logit.device)
        self._call("cwf_upsample_softmax", logit.data_ptr(), logit.stride(3), prob.data_ptr(), n, d, h, w, c, scale, self._stream())
        return prob

    def upsample_softmax_bwd(self, dprob, prob, lo_shape, c, scale, ldc_out):
        n, d, h, w = lo_shape
        dprob = dprob.contiguous()
        dl = torch.zeros((n, d, h, w, ldc_out), dtype=_f32, device=prob.device)
        ws = self.workspace("upsm_bwd", n * d * scale * h * w * c, prob.device)
        self._call("cwf_upsample_softmax_bwd", dprob.data_ptr(), prob.data_ptr(), dl.data_ptr(), ldc_out, n, d, h, w, c, scale, ws.data_ptr(), self._stream())
        return dl

    def channel_softmax(self, logit, c):
        n, d, h, w, _ = logit.shape
        prob = torch.empty((n, d, h, w, c), dtype=_f32, device=logit.device)
        self._call("cwf_channel_softmax", logit.data_ptr(), logit.stride(3), prob.data_ptr(), n * d * h * w, c, self._stream())
        return prob

    def channel_softmax_bwd(self, dprob, prob):
        dprob = dprob.contiguous()
        n, d, h, w, c = prob.shape
        dl = torch.empty_like(prob)
        self._call("cwf_channel_softmax_bwd", dprob.data_ptr(), prob.data_ptr(), dl.data_ptr(), c, n * d * h * w, c, self._stream())
        return dl

    # ------------------------------------------------------------------ K9
    def dice_ce(self, prob, label, posmask):
        """prob [N,D,H,W,C] dense channels-last, label int64 [N,D,H,W] -> (loss [1], coef [N,C,4])"""
        n, d, h, w, c = prob.shape
        v = d * h * w
        sums = self._zeros_f64((n, c, 4), prob.device)
        self._call("cwf_dice_ce_sums", prob.data_ptr(), label.data_ptr(), posmask, sums.data_ptr(), n, v, c, self._stream())
        loss = torch.empty(1, dtype=_f32, device=prob.device)
        coef = torch.empty((n, c, 4), dtype=_f32, device=prob.device)
        self._call("cwf_dice_ce_finalize", sums.data_ptr(), loss.data_ptr(), coef.data_ptr(), n, v, c, self._stream())
        return loss, coef

    def dice_ce_bwd(self, prob, label, posmask, coef, gscale):
        n, d, h, w, c = prob.shape
        dprob = torch.empty_like(prob)
        self._call("cwf_dice_ce_bwd", prob.data_ptr(), label.data_ptr(), posmask, coef.data_ptr(), gscale.data_ptr(), dprob.data_ptr(),
                   n, d * h * w, c, self._stream())
        return dprob

    # ------------------------------------------------------------------ L2-L5: the checks the supplementary loss terms share
    @staticmethod
    def _posmasks(name, posmasks):
        masks = tuple(int(m) for m in posmasks)
        if any(m < 0 or m > 0xFFFFFFFF for m in masks):
            raise ValueError("%s: a region is a 32-bit class bitmask, got %r" % (name, posmasks))
        return masks, (ctypes.c_uint32 * max(len(masks), 1))(*masks)

    @staticmethod
    def _prob_label(name, prob, label, channels):
        """prob float32 [N, D0, D1, D2, C] on the GPU with C one of `channels`, label int64 of its leading shape on the same device, both
        contiguous -> (N, V, C)"""
        if prob.dim() != 5 or prob.dtype != _f32 or not prob.is_cuda or int(prob.shape[-1]) not in channels:
            raise ValueError("%s: prob must be a float32 [N, D0, D1, D2, C] tensor on the GPU with C = %s, got %s %s"
                             % (name, " or ".join(str(c) for c in channels), tuple(prob.shape), prob.dtype))
        if tuple(label.shape) != tuple(prob.shape[:4]) or label.dtype != torch.int64 or label.device != prob.device:
            raise ValueError("%s: label must be int64 %s on the device of prob, got %s %s"
                             % (name, tuple(prob.shape[:4]), tuple(label.shape), label.dtype))
        assert prob.is_contiguous() and label.is_contiguous()
        return int(prob.shape[0]), int(prob[0, ..., 0].numel()), int(prob.shape[-1])

    @staticmethod
    def _one_float(name, what, t, device):
        if t.numel() != 1 or t.dtype != _f32 or t.device != device:
            raise ValueError("%s: %s must be a one-element float32 tensor on the device of prob" % (name, what))

    def _workspace(self, fn_name, device, *dims):
        """the uint8 workspace of the size the library's `fn_name`(*dims) asks for.  No host synchronisation: it comes from torch's
        allocator."""
        nbytes = getattr(self.lib, fn_name)(*dims)
        if nbytes < 0:
            raise _lib.CwfError("%s%r failed with status %d" % (fn_name, dims, nbytes))
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device)

    # ------------------------------------------------------------------ L2 (boundary loss)
    def signed_distance(self, label, posmasks=REGION_MASKS):
        """label int64 [N, D0, D1, D2] -> phi float32 [N, R, D0, D1, D2]: the exact Euclidean signed distance map of every region
        (class bitmask) of `posmasks`, sqrt(q) outside and 1 - sqrt(q) inside, rounded once from float64; zeros where a region is empty
        or fills the volume (cwf_signed_distance)."""
        if label.dim() != 4 or label.dtype != torch.int64 or not label.is_cuda:
            raise ValueError("signed_distance: label must be an int64 [N, D0, D1, D2] tensor on the GPU")
        masks, cm = self._posmasks("signed_distance", posmasks)
        label = label.contiguous()
        n, d0, d1, d2 = (int(s) for s in label.shape)
        ws = self._workspace("cwf_signed_distance_workspace", label.device, n, len(masks), d0, d1, d2)
        phi = torch.empty((n, len(masks), d0, d1, d2), dtype=_f32, device=label.device)
        self._call("cwf_signed_distance", label.data_ptr(), ctypes.addressof(cm), phi.data_ptr(), n, len(masks), d0, d1, d2, ws.data_ptr(),
                   self._stream())
        return phi

    def boundary_loss(self, prob, phi, posmasks, weight):
        """prob [N,D0,D1,D2,C] dense channels-last, phi [N,R,D0,D1,D2], weight a one-float device tensor -> (loss [1], coef [1])"""
        masks, cm = self._posmasks("boundary_loss", posmasks)
        n, c = int(prob.shape[0]), int(prob.shape[-1])
        v = int(prob[0, ..., 0].numel())
        if tuple(phi.shape) != (n, len(masks)) + tuple(prob.shape[1:4]) or phi.dtype != _f32 or prob.dtype != _f32:
            raise ValueError("boundary_loss: phi must be float32 [N, R, D0, D1, D2] for prob [N, D0, D1, D2, C], got %s and %s"
                             % (tuple(phi.shape), tuple(prob.shape)))
        self._one_float("boundary_loss", "weight", weight, prob.device)
        assert prob.is_contiguous() and phi.is_contiguous()
        s = self._zeros_f64((1,), prob.device)
        self._call("cwf_boundary_sums", prob.data_ptr(), phi.data_ptr(), ctypes.addressof(cm), s.data_ptr(), n, len(masks), v, c, self._stream())
        loss = torch.empty(1, dtype=_f32, device=prob.device)
        coef = torch.empty(1, dtype=_f32, device=prob.device)
        self._call("cwf_boundary_finalize", s.data_ptr(), weight.data_ptr(), loss.data_ptr(), coef.data_ptr(), n, len(masks), v, self._stream())
        return loss, coef

    def boundary_loss_bwd(self, prob, phi, posmasks, coef, gscale):
        """-> dprob like prob: (gscale * coef) * (sum of phi over the regions holding the class)"""
        masks, cm = self._posmasks("boundary_loss_bwd", posmasks)
        n, c = int(prob.shape[0]), int(prob.shape[-1])
        dprob = torch.empty_like(prob)
        self._call("cwf_boundary_bwd", phi.data_ptr(), ctypes.addressof(cm), coef.data_ptr(), gscale.data_ptr(), dprob.data_ptr(), n, len(masks),
                   int(prob[0, ..., 0].numel()), c, self._stream())
        return dprob

    # ------------------------------------------------------------------ L3 (top-k cross-entropy)
    @staticmethod
    def _topk_args(name, prob, label, posmask):
        n, v, c = HipBackend._prob_label(name, prob, label, (2, 4))
        posmask = int(posmask)
        if posmask < 0 or posmask > 0xFFFFFFFF:
            raise ValueError("%s: posmask is a 32-bit class bitmask, got %r" % (name, posmask))
        return n, v, c, posmask

    def topk_ce(self, prob, label, posmask, k, weight):
        """prob [N,D0,D1,D2,C] dense channels-last (C = 4 or 2), label int64 [N,D0,D1,D2], k voxels of the whole batch, weight a
        one-float device tensor -> (loss [1], coef [4]): weight x mean of -log p_t over the k hardest voxels by an exact radix select
        on the device (cwf_topk_ce)."""
        n, v, c, posmask = self._topk_args("topk_ce", prob, label, posmask)
        k = int(k)
        if k < 1 or k > n * v:
            raise ValueError("topk_ce: k must lie in 1..N V = %d, got %d" % (n * v, k))
        self._one_float("topk_ce", "weight", weight, prob.device)
        ws = self._workspace("cwf_topk_ce_workspace", prob.device, n, v)
        loss = torch.empty(1, dtype=_f32, device=prob.device)
        coef = torch.empty(4, dtype=_f32, device=prob.device)
        self._call("cwf_topk_ce", prob.data_ptr(), label.data_ptr(), posmask, k, weight.data_ptr(), loss.data_ptr(), coef.data_ptr(), n, v, c,
                   ws.data_ptr(), self._stream())
        return loss, coef

    def topk_ce_bwd(self, prob, label, posmask, coef, gscale):
        """-> dprob like prob: (gscale * coef[0]) * (-1 / max(pc, 1e-7)) at the target class of the voxels below tau, that times coef[1]
        on the ties at tau, +0 elsewhere"""
        n, v, c, posmask = self._topk_args("topk_ce_bwd", prob, label, posmask)
        dprob = torch.empty_like(prob)
        self._call("cwf_topk_ce_bwd", prob.data_ptr(), label.data_ptr(), posmask, coef.data_ptr(), gscale.data_ptr(), dprob.data_ptr(), n, v, c,
                   self._stream())
        return dprob

    # ------------------------------------------------------------------ L4 (focal Tversky + focal cross-entropy)
    @staticmethod
    def _focal_args(name, prob, label, posmasks, params):
        """-> (N, V, masks, the uint32 array, the cwf_focal_params struct); every check the C entry makes, made before any call"""
        n, v, _ = HipBackend._prob_label(name, prob, label, (4,))
        masks, cm = HipBackend._posmasks(name, posmasks)
        p = check_focal_params(masks, **params)
        cp = _lib.FocalParams(p["fn"], p["fp"], p["exponent"], p["smooth"], p["gamma"], p["ce_ratio"], (ctypes.c_double * 4)(*p["class_weight"]))
        return n, v, masks, cm, cp

    def focal_loss(self, prob, label, posmasks, params, weight):
        """prob [N,D0,D1,D2,4] dense channels-last, label int64 [N,D0,D1,D2], posmasks R <= 8 class bitmasks over bits 0..3, params a
        dict (fn, fp, exponent, smooth, gamma, ce_ratio, class_weight), weight a one-float device tensor -> (loss [1], coef [2 R + 1]):
        weight x (focal Tversky of the regions + ce_ratio x focal cross-entropy), sums over the whole batch (cwf_focal_loss)."""
        n, v, masks, cm, cp = self._focal_args("focal_loss", prob, label, posmasks, params)
        self._one_float("focal_loss", "weight", weight, prob.device)
        ws = self._workspace("cwf_focal_workspace", prob.device, n, v, len(masks))
        loss = torch.empty(1, dtype=_f32, device=prob.device)
        coef = torch.empty(2 * len(masks) + 1, dtype=_f32, device=prob.device)
        self._call("cwf_focal_loss", prob.data_ptr(), label.data_ptr(), ctypes.addressof(cm), len(masks), ctypes.addressof(cp), weight.data_ptr(),
                   loss.data_ptr(), coef.data_ptr(), n, v, 4, ws.data_ptr(), self._stream())
        return loss, coef

    def focal_loss_bwd(self, prob, label, posmasks, params, coef, gscale):
        """-> dprob like prob: gscale x (the sum of t_r coef[2 r] + coef[2 r + 1] over the regions holding the class, plus coef[2 R] k_y
        d/dq[-(1 - q)^gamma ln q] at the label's class where 1e-7 <= p_y <= 1); every element written (cwf_focal_loss_bwd)"""
        n, v, masks, cm, cp = self._focal_args("focal_loss_bwd", prob, label, posmasks, params)
        if coef.numel() != 2 * len(masks) + 1 or coef.dtype != _f32 or coef.device != prob.device or not coef.is_contiguous():
            raise ValueError("focal_loss_bwd: coef must be the float32 [2 R + 1] tensor focal_loss returned")
        dprob = torch.empty_like(prob)
        self._call("cwf_focal_loss_bwd", prob.data_ptr(), label.data_ptr(), ctypes.addressof(cm), len(masks), ctypes.addressof(cp), coef.data_ptr(),
                   gscale.data_ptr(), dprob.data_ptr(), n, v, 4, self._stream())
        return dprob

    # ------------------------------------------------------------------ L5 (Lovasz-Softmax)
    def lovasz(self, prob, label, posmasks, only_present, weight):
        """prob [N,D0,D1,D2,4] dense channels-last, label int64 [N,D0,D1,D2], posmasks 1..8 class bitmasks in 1..15, weight a one-float
        device tensor -> (loss [1], coef [4], vcoef [R, N V]): weight x the mean over the counted regions of the Lovasz extension of the
        Jaccard loss, by an exact sort of the errors of the whole batch on the device (cwf_lovasz)."""
        n, v, _ = self._prob_label("lovasz", prob, label, (4,))
        masks, only_present = check_lovasz_params(posmasks, only_present)
        self._one_float("lovasz", "weight", weight, prob.device)
        if n * v > 0x7FFFFFFF:
            raise ValueError("lovasz: at most 2^31 - 1 voxels in the batch, got %d" % (n * v))
        cm = (ctypes.c_uint32 * len(masks))(*masks)
        ws = self._workspace("cwf_lovasz_workspace", prob.device, n, v, len(masks))
        loss = torch.empty(1, dtype=_f32, device=prob.device)
        coef = torch.empty(4, dtype=_f32, device=prob.device)
        vcoef = torch.empty((len(masks), n * v), dtype=_f32, device=prob.device)
        self._call("cwf_lovasz", prob.data_ptr(), label.data_ptr(), ctypes.addressof(cm), len(masks), int(only_present), weight.data_ptr(),
                   loss.data_ptr(), coef.data_ptr(), vcoef.data_ptr(), n, v, ws.data_ptr(), self._stream())
        return loss, coef, vcoef

    def lovasz_bwd(self, vcoef, posmasks, coef, gscale, shape):
        """-> dprob float32 `shape` = [N,D0,D1,D2,4]: (gscale x coef[0]) x vcoef[r] summed over the regions holding the class, ascending
        r; every element written (cwf_lovasz_bwd)"""
        masks, _ = check_lovasz_params(posmasks)
        shape = tuple(int(s) for s in shape)
        if len(shape) != 5 or shape[-1] != 4:
            raise ValueError("lovasz_bwd: shape must be [N, D0, D1, D2, 4], got %r" % (shape,))
        n, v = shape[0], shape[1] * shape[2] * shape[3]
        if not vcoef.is_cuda or tuple(vcoef.shape) != (len(masks), n * v) or vcoef.dtype != _f32 or not vcoef.is_contiguous():
            raise ValueError("lovasz_bwd: vcoef must be the float32 [R, N V] tensor lovasz returned")
        if coef.numel() != 4 or coef.dtype != _f32 or coef.device != vcoef.device or gscale.numel() != 1 or gscale.dtype != _f32 \
                or gscale.device != vcoef.device:
            raise ValueError("lovasz_bwd: coef must be the float32 [4] tensor lovasz returned and gscale one float32, on the device of vcoef")
        cm = (ctypes.c_uint32 * len(masks))(*masks)
        dprob = torch.empty(shape, dtype=_f32, device=vcoef.device)
        self._call("cwf_lovasz_bwd", vcoef.data_ptr(), ctypes.addressof(cm), len(masks), coef.data_ptr(), gscale.data_ptr(), dprob.data_ptr(),
                   n, v, self._stream())
        return dprob

    def head_loss(self, logits, label, posmasks, scale):
        """Fused head -> loss forward: logits = up to 3 low-res [N,d,h,w,ldc] tensors (2 channels used), label int64 [N,D,H,W].
        -> (total [1], loss [nm], coef [nm,N,2,4])"""
        nm = len(logits)
        n, d, h, w, _ = logits[0].shape
        ldc = logits[0].stride(3)                  # (channel slices of one grouped logit buffer: rows ldc floats apart)
        assert all(t.shape == logits[0].shape and t.stride() == logits[0].stride() and t.stride(4) == 1 for t in logits) and label.is_contiguous()
        assert logits[0].stride(2) == w * ldc and logits[0].stride(1) == h * w * ldc and logits[0].stride(0) == d * h * w * ldc
        dev = logits[0].device
        sums = self._zeros_f64((nm, n, 2, 4), dev)
        ptrs = (ctypes.c_void_p * nm)(*[t.data_ptr() for t in logits])
        masks = (ctypes.c_uint32 * nm)(*[int(m) for m in posmasks])
        self._call("cwf_head_loss_sums", ctypes.addressof(ptrs), nm, ldc, ctypes.addressof(masks), label.data_ptr(), sums.data_ptr(), n, d, h, w, scale, self._stream())
        loss = torch.empty(nm, dtype=_f32, device=dev)
        total = torch.empty(1, dtype=_f32, device=dev)
        coef = torch.empty((nm, n, 2, 4), dtype=_f32, device=dev)
        self._call("cwf_dice_ce_finalize_multi", sums.data_ptr(), loss.data_ptr(), coef.data_ptr(), total.data_ptr(), nm, n,
                   d * h * w * scale ** 3, 2, self._stream())
        return total, loss, coef

    def head_loss_bwd(self, logits, label, posmasks, scale, coef, gscale, grouped_out=None):
        """-> list of d(logit) tensors.  grouped_out = (buffer [N,d,h,w,nm*ca], ca): the gradients are written as channel groups of
        that ONE buffer (ca channels each: 2 values + zeroed padding) and the returned tensors are its slices."""
        nm = len(logits)
        n, d, h, w, ca = logits[0].shape
        ldc = logits[0].stride(3)
        dev = logits[0].device
        if grouped_out is None:
            dls = [torch.empty((n, d, h, w, ca), dtype=_f32, device=dev) for _ in logits]
            dl_ca, dl_ldc = ca, ca
        else:
            buf, dl_ca = grouped_out
            dl_ldc = buf.stride(3)
            dls = [buf[..., m * dl_ca:(m + 1) * dl_ca] for m in range(nm)]
        ws = self.workspace("head_loss_bwd", nm * n * d * scale * h * w * 2, dev)
        ptrs = (ctypes.c_void_p * nm)(*[t.data_ptr() for t in logits])
        dptrs = (ctypes.c_void_p * nm)(*[t.data_ptr() for t in dls])
        masks = (ctypes.c_uint32 * nm)(*[int(m) for m in posmasks])
        self._call("cwf_head_loss_bwd_ex", ctypes.addressof(ptrs), nm, ldc, ctypes.addressof(masks), label.data_ptr(), coef.data_ptr(), gscale.data_ptr(),
                   ctypes.addressof(dptrs), dl_ca, dl_ldc, ws.data_ptr(), n, d, h, w, scale, self._stream())
        return dls

    # ------------------------------------------------------------------ N1 (sliding-window inference glue)
    def stitch_windows(self, out8, nb):
        """out8: the model's output for the 8 windows stacked along the batch, logical [8*nb,4,128,128,128] over channels-last memory
        -> stitched [nb,4,240,240,155] (predict_overlap.py:49-58, incl. the depth-axis offset quirk)"""
        if not (torch.is_tensor(out8) and out8.is_cuda and out8.dtype == _f32 and int(nb) >= 1
                and tuple(out8.shape) == (8 * int(nb), 4, 128, 128, 128)):
            raise ValueError("stitch_windows: out8 must be a CUDA float32 [8 * nb, 4, 128, 128, 128] tensor with nb >= 1, got %s %s and nb = %r"
                             % (getattr(out8, "dtype", type(out8)), tuple(getattr(out8, "shape", ())), nb))
        nb = int(nb)
        w = out8.permute(0, 2, 3, 4, 1)
        if not w.is_contiguous():
            w = w.contiguous()
        y = torch.empty((nb, 4, 240, 240, 155), dtype=_f32, device=out8.device)
        self._call("cwf_stitch_windows", w.data_ptr(), y.data_ptr(), nb, self._stream())
        return y

    def argmax_dice(self, prob, target=None, miou=False, counts=False):
        """prob: CUDA float32 [B,4,...] with at least one spatial axis, of any strides (contiguous and channels-last memory are read in
        place, anything else is copied) -> (seg int64 [B,...], [WT, TC, ET] Dice tensor or None); target: None or an int64 tensor
        [B,...] on prob's device; with miou=True (target required) a third result: the [class 1, 2, 3] IoU tensor of
        tools.softmax_mIOU_score (utils/tools.py:50-61).  The argmax is torch.argmax's: the first maximum, a NaN being the maximum.
        counts=True (target required) appends the int64 device tensor the ratios were formed from: rows of (|o & t|, |o|, |t|) for WT, TC,
        ET and, with miou, class 1, 2, 3 -- [3, 3] or [6, 3]."""
        if not (torch.is_tensor(prob) and prob.is_cuda and prob.dtype == _f32 and prob.dim() >= 3 and prob.shape[1] == 4 and prob.numel() > 0):
            raise ValueError("argmax_dice: prob must be a non-empty CUDA float32 [B, 4, ...] tensor with at least one spatial axis, got %s %s"
                             % (getattr(prob, "dtype", type(prob)), tuple(getattr(prob, "shape", ()))))
        b = prob.shape[0]
        sp = tuple(prob.shape[2:])
        if target is not None and not (torch.is_tensor(target) and target.dtype == torch.int64 and target.device == prob.device
                                       and tuple(target.shape) == (b,) + sp):
            raise ValueError("argmax_dice: target must be an int64 %r tensor on the device of prob, got %s %s on %s"
                             % ((b,) + sp, getattr(target, "dtype", type(target)), tuple(getattr(target, "shape", ())),
                                getattr(target, "device", None)))
        if miou and target is None:
            raise ValueError("argmax_dice: miou=True needs a target")
        if counts and target is None:
            raise ValueError("argmax_dice: counts=True needs a target")
        want_counts = bool(counts)
        v = 1
        for d in sp:
            v *= d
        if prob.is_contiguous():
            sb, sc, sv = 4 * v, v, 1
        elif prob.movedim(1, -1).is_contiguous():              # channels-last memory of any rank (5-D: permute(0, 2, 3, 4, 1))
            sb, sc, sv = 4 * v, 1, 4
        else:
            prob = prob.contiguous(); sb, sc, sv = 4 * v, v, 1
        seg = torch.empty((b,) + sp, dtype=torch.int64, device=prob.device)
        counts = None
        if target is not None:
            target = target.contiguous()
            counts = torch.zeros((6 if miou else 3, 3), dtype=torch.int64, device=prob.device)
        if miou:
            self._call("cwf_argmax_metrics", prob.data_ptr(), sb, sc, sv, target.data_ptr(), seg.data_ptr(), counts.data_ptr(), b, v, self._stream())
        else:
            self._call("cwf_argmax_dice", prob.data_ptr(), sb, sc, sv, _p(target), seg.data_ptr(), _p(counts), b, v, self._stream())
        dice = None
        if counts is not None:
            c = counts.double()
            dice = (2 * c[:3, 0] + 1e-8) / (c[:3, 1] + c[:3, 2] + 1e-8)       # tools.dice_score (utils/tools.py:44-47)
            if miou:
                iou = (c[3:, 0] + 1e-8) / (c[3:, 1] + c[3:, 2] - c[3:, 0] + 1e-8)   # tools.mIOU (utils/tools.py:50-53): |o & t| / |o | t|
                return (seg, dice, iou, counts) if want_counts else (seg, dice, iou)
        return (seg, dice, counts) if want_counts else (seg, dice)

    def region_bits(self, labels):
        """int64 label map (any shape) -> uint8 region bits of tools.softmax_output_dice: bit 0 WT, bit 1 TC, bit 2 ET (cwf_region_bits)"""
        if not (torch.is_tensor(labels) and labels.dtype == torch.int64 and labels.is_cuda):
            raise ValueError("region_bits: labels must be a CUDA int64 tensor, got %s on %s"
                             % (getattr(labels, "dtype", type(labels)), getattr(labels, "device", None)))
        labels = labels.contiguous()
        bits = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
        if labels.numel():
            self._call("cwf_region_bits", labels.data_ptr(), bits.data_ptr(), labels.numel(), self._stream())
        return bits

    def hausdorff(self, a_bits, b_bits, R, spacing=None, connectivity=1, all_border=False):
        """medpy's hd / hd95 of the masks a, b ([B, D0, D1, D2] uint8 region bits or bool, bit r = region r < R <= 8) on the device:
        -> (hd [B, R] float64, hd95 [B, R] float64, counts [B, R, 4] int64 = |A|, |B|, |dA|, |dB|); NaN distances where a mask is
        empty.  spacing: None, a scalar or three per-axis values; all_border: every mask voxel is a border voxel (medpy on [1, ...]
        arrays).  No host synchronisation: the workspace comes from torch's allocator on the current stream."""
        if a_bits.dtype == torch.bool:
            a_bits = a_bits.view(torch.uint8)
        if b_bits.dtype == torch.bool:
            b_bits = b_bits.view(torch.uint8)
        if a_bits.dim() != 4 or tuple(a_bits.shape) != tuple(b_bits.shape) or a_bits.dtype != torch.uint8 or b_bits.dtype != torch.uint8:
            raise ValueError("hausdorff: a_bits and b_bits must be uint8 / bool tensors of one [B, D0, D1, D2] shape")
        if spacing is None:
            sp = (1.0, 1.0, 1.0)
        elif isinstance(spacing, (int, float)):
            sp = (float(spacing),) * 3
        else:
            sp = tuple(float(s) for s in spacing)
            if len(sp) != 3:
                raise ValueError("hausdorff: spacing needs one value per axis, got %r" % (spacing,))
        a_bits, b_bits = a_bits.contiguous(), b_bits.contiguous()
        nb, d0, d1, d2 = (int(s) for s in a_bits.shape)
        dev = a_bits.device
        nbytes = self.lib.cwf_hausdorff_workspace(nb, int(R), d0, d1, d2)
        if nbytes < 0:
            raise _lib.CwfError("cwf_hausdorff_workspace failed with status %d (B=%d R=%d %dx%dx%d)" % (nbytes, nb, R, d0, d1, d2))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        hd = torch.empty((nb, int(R)), dtype=torch.float64, device=dev)
        hd95 = torch.empty((nb, int(R)), dtype=torch.float64, device=dev)
        counts = torch.empty((nb, int(R), 4), dtype=torch.int64, device=dev)
        self._call("cwf_hausdorff", a_bits.data_ptr(), b_bits.data_ptr(), nb, int(R), d0, d1, d2, sp[0], sp[1], sp[2], int(connectivity),
                   int(bool(all_border)), hd.data_ptr(), hd95.data_ptr(), counts.data_ptr(), ws.data_ptr(), int(nbytes), self._stream())
        return hd, hd95, counts

    @staticmethod
    def _tolerances(name, tolerances):
        """NSD tolerances -> (tuple of floats, ctypes double array or None); at most 4, each >= 0 (+inf allowed), no NaN."""
        tol = tuple(float(t) for t in (tolerances if tolerances is not None else ()))
        if len(tol) > 4:
            raise ValueError("%s: at most 4 tolerances per call, got %d" % (name, len(tol)))
        if any(not t >= 0.0 for t in tol):
            raise ValueError("%s: tolerances must be >= 0 (and not NaN), got %r" % (name, tol))
        return tol, ((ctypes.c_double * len(tol))(*tol) if tol else None)

    def surface_metrics(self, a_bits, b_bits, R, tolerances=(), spacing=None, connectivity=1, all_border=False):
        """Normalised surface Dice at up to four `tolerances` and medpy's asd / assd of the masks a, b, with hd / hd95, on the borders
        and exact distances of `hausdorff` (same arguments; cwf_surface_metrics): -> dict of hd, hd95 [B, R], asd [B, R, 2] = mean
        distance dA -> dB, dB -> dA, assd [B, R], nsd [B, R, T] float64, within [B, R, T, 2] int64 = border voxels of A, of B within the
        tolerance, counts [B, R, 4] int64 = |A|, |B|, |dA|, |dB|.  nsd = (within[..., 0] + within[..., 1]) / (|dA| + |dB|): the
        voxel-border form, with unit spacing every tolerance < 1 counts coincident border voxels only.  NaN floats and zero within
        where a mask is empty.  Every output is bit-identical from run to run.  No host synchronisation: the workspace comes from
        torch's allocator on the current stream."""
        if torch.is_tensor(a_bits) and a_bits.dtype == torch.bool:
            a_bits = a_bits.view(torch.uint8)
        if torch.is_tensor(b_bits) and b_bits.dtype == torch.bool:
            b_bits = b_bits.view(torch.uint8)
        if not torch.is_tensor(a_bits) or not torch.is_tensor(b_bits) or a_bits.dim() != 4 or tuple(a_bits.shape) != tuple(b_bits.shape) \
                or a_bits.dtype != torch.uint8 or b_bits.dtype != torch.uint8:
            raise ValueError("surface_metrics: a_bits and b_bits must be uint8 / bool tensors of one [B, D0, D1, D2] shape")
        if not a_bits.is_cuda or a_bits.device != b_bits.device or a_bits.numel() == 0:
            raise ValueError("surface_metrics: a_bits and b_bits must be non-empty CUDA tensors on one device")
        if not 1 <= int(R) <= 8:
            raise ValueError("surface_metrics: R must lie in 1..8, got %r" % (R,))
        if int(connectivity) not in (1, 2, 3):
            raise ValueError("surface_metrics: connectivity must be 1, 2 or 3, got %r" % (connectivity,))
        tol, tau = self._tolerances("surface_metrics", tolerances)
        if spacing is None:
            sp = (1.0, 1.0, 1.0)
        elif isinstance(spacing, (int, float)):
            sp = (float(spacing),) * 3
        else:
            sp = tuple(float(s) for s in spacing)
            if len(sp) != 3:
                raise ValueError("surface_metrics: spacing needs one value per axis, got %r" % (spacing,))
        a_bits, b_bits = a_bits.contiguous(), b_bits.contiguous()
        nb, d0, d1, d2 = (int(s) for s in a_bits.shape)
        R, T, dev = int(R), len(tol), a_bits.device
        nbytes = self.lib.cwf_surface_metrics_workspace(nb, R, d0, d1, d2)
        if nbytes < 0:
            raise _lib.CwfError("cwf_surface_metrics_workspace failed with status %d (B=%d R=%d %dx%dx%d)" % (nbytes, nb, R, d0, d1, d2))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        out = {"hd": torch.empty((nb, R), dtype=torch.float64, device=dev), "hd95": torch.empty((nb, R), dtype=torch.float64, device=dev),
               "asd": torch.empty((nb, R, 2), dtype=torch.float64, device=dev), "assd": torch.empty((nb, R), dtype=torch.float64, device=dev),
               "nsd": torch.empty((nb, R, T), dtype=torch.float64, device=dev),
               "within": torch.empty((nb, R, T, 2), dtype=torch.int64, device=dev),
               "counts": torch.empty((nb, R, 4), dtype=torch.int64, device=dev)}
        self._call("cwf_surface_metrics", a_bits.data_ptr(), b_bits.data_ptr(), nb, R, d0, d1, d2, sp[0], sp[1], sp[2], int(connectivity),
                   int(bool(all_border)), tau, T, out["hd"].data_ptr(), out["hd95"].data_ptr(), out["asd"].data_ptr(),
                   out["assd"].data_ptr(), out["within"].data_ptr() if T else None, out["nsd"].data_ptr() if T else None,
                   out["counts"].data_ptr(), ws.data_ptr(), int(nbytes), self._stream())
        return out

    # ------------------------------------------------------------------ N6 connected components and label-map post-processing
    def components(self, bits, R, connectivity=1):
        """Connected components of every region of bits ([B, D0, D1, D2] uint8 region bits or bool, bit r = region r < R <= 8) under the
        6/18/26-neighbour footprint (connectivity 1/2/3), numbered as scipy.ndimage.label numbers them (cwf_components):
        -> (labels [B, R, D0, D1, D2] int32, sizes [B, R, cap] int32 with cap = (V + 1) // 2 and zeros beyond the last component,
        count [B, R] int32, largest [B, R, 2] int32 = (label, size), ties to the lowest label).  No host synchronisation: the workspace
        comes from torch's allocator on the current stream."""
        if torch.is_tensor(bits) and bits.dtype == torch.bool:
            bits = bits.view(torch.uint8)
        if not torch.is_tensor(bits) or bits.dim() != 4 or bits.dtype != torch.uint8 or not bits.is_cuda or bits.numel() == 0:
            raise ValueError("components: bits must be a non-empty CUDA uint8 / bool tensor of shape [B, D0, D1, D2]")
        if not 1 <= int(R) <= 8:
            raise ValueError("components: R must lie in 1..8, got %r" % (R,))
        if int(connectivity) not in (1, 2, 3):
            raise ValueError("components: connectivity must be 1, 2 or 3, got %r" % (connectivity,))
        bits = bits.contiguous()
        nb, d0, d1, d2 = (int(s) for s in bits.shape)
        R, dev = int(R), bits.device
        nbytes = self.lib.cwf_components_workspace(nb, R, d0, d1, d2)
        if nbytes < 0:
            raise _lib.CwfError("cwf_components_workspace failed with status %d (B=%d R=%d %dx%dx%d)" % (nbytes, nb, R, d0, d1, d2))
        cap = (d0 * d1 * d2 + 1) // 2
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        labels = torch.empty((nb, R, d0, d1, d2), dtype=torch.int32, device=dev)
        sizes = torch.empty((nb, R, cap), dtype=torch.int32, device=dev)
        count = torch.empty((nb, R), dtype=torch.int32, device=dev)
        largest = torch.empty((nb, R, 2), dtype=torch.int32, device=dev)
        self._call("cwf_components", bits.data_ptr(), nb, R, d0, d1, d2, int(connectivity), labels.data_ptr(), sizes.data_ptr(),
                   count.data_ptr(), largest.data_ptr(), ws.data_ptr(), int(nbytes), self._stream())
        return labels, sizes, count, largest

    def postprocess_labels(self, seg, labels, sizes, largest, wt_region=0, et_region=2, min_component=0, keep_largest=False,
                           et_min_component=0, et_min_voxels=0, et_replace=1):
        """The post-processing policy of predict_overlap.postprocess on a CUDA int64 label map seg [B, D0, D1, D2] (classes 0..3), from
        the `components` results of its region bits (cwf_postprocess_labels): -> (processed map, stats [B, 4] int64 = WT voxels removed,
        WT components removed, ET voxels relabelled, ET voxels remaining).  No host synchronisation."""
        if not torch.is_tensor(seg) or seg.dim() != 4 or seg.dtype != torch.int64 or not seg.is_cuda or seg.numel() == 0:
            raise ValueError("postprocess_labels: seg must be a non-empty CUDA int64 tensor of shape [B, D0, D1, D2]")
        nb, d0, d1, d2 = (int(s) for s in seg.shape)
        if labels.dim() != 5 or labels.dtype != torch.int32 or labels.shape[0] != nb or tuple(labels.shape[2:]) != (d0, d1, d2):
            raise ValueError("postprocess_labels: labels must be the int32 [B, R, D0, D1, D2] result of components for this map")
        R, cap = int(labels.shape[1]), (d0 * d1 * d2 + 1) // 2
        if tuple(sizes.shape) != (nb, R, cap) or sizes.dtype != torch.int32 or tuple(largest.shape) != (nb, R, 2) or largest.dtype != torch.int32:
            raise ValueError("postprocess_labels: sizes / largest must be the int32 [B, R, cap] / [B, R, 2] results of components")
        if not (0 <= int(wt_region) < R and 0 <= int(et_region) < R):
            raise ValueError("postprocess_labels: region indices must lie in [0, %d), got %r and %r" % (R, wt_region, et_region))
        if min(int(min_component), int(et_min_component), int(et_min_voxels)) < 0:
            raise ValueError("postprocess_labels: thresholds must be >= 0")
        if int(et_replace) not in (0, 1, 2):
            raise ValueError("postprocess_labels: et_replace must be 0, 1 or 2, got %r" % (et_replace,))
        seg, labels, sizes, largest = seg.contiguous(), labels.contiguous(), sizes.contiguous(), largest.contiguous()
        out = torch.empty_like(seg)
        stats = torch.empty((nb, 4), dtype=torch.int64, device=seg.device)
        ws = torch.empty((nb, 4), dtype=torch.int64, device=seg.device)          # CWF_POSTPROCESS_WS_BYTES
        self._call("cwf_postprocess_labels", seg.data_ptr(), out.data_ptr(), labels.data_ptr(), sizes.data_ptr(), largest.data_ptr(), nb, R,
                   d0, d1, d2, int(wt_region), int(et_region), int(min_component), int(bool(keep_largest)), int(et_min_component),
                   int(et_min_voxels), int(et_replace), stats.data_ptr(), ws.data_ptr(), self._stream())
        return out, stats

    def label_metrics(self, seg, target, counts=False):
        """(dice [3], iou [3]) float64 device tensors of two int64 label maps of one shape: WT / TC / ET Dice of tools.softmax_output_dice
        and class 1 / 2 / 3 IoU of tools.softmax_mIOU_score, by the formulas of argmax_dice (cwf_label_metrics).  counts=True appends the
        int64 [6, 3] device tensor they were formed from: (|o & t|, |o|, |t|) of WT, TC, ET, class 1, 2, 3."""
        for name, t in (("seg", seg), ("target", target)):
            if not (torch.is_tensor(t) and t.dtype == torch.int64 and t.is_cuda):
                raise ValueError("label_metrics: %s must be a CUDA int64 tensor, got %s on %s"
                                 % (name, getattr(t, "dtype", type(t)), getattr(t, "device", None)))
        if tuple(seg.shape) != tuple(target.shape) or seg.device != target.device or seg.numel() == 0:
            raise ValueError("label_metrics: seg and target must have one non-empty shape and one device, got %r on %s and %r on %s"
                             % (tuple(seg.shape), seg.device, tuple(target.shape), target.device))
        seg, target = seg.contiguous(), target.contiguous()
        table = torch.zeros((6, 3), dtype=torch.int64, device=seg.device)
        self._call("cwf_label_metrics", seg.data_ptr(), target.data_ptr(), table.data_ptr(), seg.numel(), self._stream())
        c = table.double()
        dice, iou = (2 * c[:3, 0] + 1e-8) / (c[:3, 1] + c[:3, 2] + 1e-8), (c[3:, 0] + 1e-8) / (c[3:, 1] + c[3:, 2] - c[3:, 0] + 1e-8)
        return (dice, iou, table) if counts else (dice, iou)

    # ------------------------------------------------------------------ N7 lesion-wise Dice and HD95
    @staticmethod
    def _region_bits_arg(name, bits):
        if torch.is_tensor(bits) and bits.dtype == torch.bool:
            bits = bits.view(torch.uint8)
        if not torch.is_tensor(bits) or bits.dim() != 4 or bits.dtype != torch.uint8 or not bits.is_cuda or bits.numel() == 0:
            raise ValueError("%s: bits must be a non-empty CUDA uint8 / bool tensor of shape [B, D0, D1, D2]" % name)
        return bits.contiguous()

    def dilate_bits(self, bits, connectivity=2, iterations=1):
        """bits ([B, D0, D1, D2] uint8 region bits or bool) dilated `iterations` (0..8) times with the 6/18/26-neighbour footprint
        (connectivity 1/2/3), every bit on its own, out-of-volume voxels unset: scipy.ndimage.binary_dilation(..., iterations) per bit
        (cwf_dilate_bits).  Returns a new uint8 tensor.  No host synchronisation."""
        bits = self._region_bits_arg("dilate_bits", bits)
        if int(connectivity) not in (1, 2, 3):
            raise ValueError("dilate_bits: connectivity must be 1, 2 or 3, got %r" % (connectivity,))
        if not 0 <= int(iterations) <= 8:
            raise ValueError("dilate_bits: iterations must lie in 0..8, got %r" % (iterations,))
        nb, d0, d1, d2 = (int(s) for s in bits.shape)
        out = torch.empty_like(bits)
        ws = torch.empty(bits.numel() if int(iterations) >= 2 else 0, dtype=torch.uint8, device=bits.device)
        self._call("cwf_dilate_bits", bits.data_ptr(), out.data_ptr(), nb, d0, d1, d2, int(connectivity), int(iterations),
                   ws.data_ptr() if ws.numel() else None, ws.numel(), self._stream())
        return out

    def lesionwise(self, pred_bits, gt_bits, R, dilation=3, min_lesion_voxels=50, penalty=374.0, nsd_tolerances=()):
        """Lesion-wise Dice and HD95 of every sample and region r < R <= 8 of two [B, D0, D1, D2] uint8 region-bit tensors, as
        predict_overlap.lesionwise_metrics defines them (cwf_lesionwise): -> (summary [B, R, 2] float64 = lw_dice, lw_hd95;
        counts [B, R, 6] int64 = G, kept, matched components, FP, FN, P; overflow [B, R] int32; table [B, R, 64, 4] int64 = gt_vol,
        pred_vol, inter, touching components per lesion; lesion_hd95 [B, R, 64] float64).  Where a (sample, region) has more than 64
        lesions its overflow flag is 1 and its other outputs stay zero.  The call waits on the stream once (the lesion counts size the
        HD95 launches), so it cannot be captured into a graph.
        nsd_tolerances: up to four tolerances; non-empty -> cwf_lesionwise_ex, and the tuple gains lesion_nsd [B, R, 64, T] float64 (the
        normalised surface Dice of (pred_g, lesion g) as `surface_metrics` defines it, 0 for a lesion nothing touches) and lw_nsd
        [B, R, T] float64 ((sum over kept lesions of nsd_g) / (kept + FP), 1 if that is 0 / 0); the first five are unchanged."""
        pred_bits = self._region_bits_arg("lesionwise", pred_bits)
        gt_bits = self._region_bits_arg("lesionwise", gt_bits)
        if tuple(pred_bits.shape) != tuple(gt_bits.shape) or pred_bits.device != gt_bits.device:
            raise ValueError("lesionwise: pred_bits and gt_bits must have one shape and device, got %r and %r"
                             % (tuple(pred_bits.shape), tuple(gt_bits.shape)))
        if not 1 <= int(R) <= 8:
            raise ValueError("lesionwise: R must lie in 1..8, got %r" % (R,))
        if not 0 <= int(dilation) <= 8:
            raise ValueError("lesionwise: dilation must lie in 0..8, got %r" % (dilation,))
        if int(min_lesion_voxels) < 0 or not 0.0 <= float(penalty) < 1e300:
            raise ValueError("lesionwise: min_lesion_voxels and penalty must be >= 0 (and finite), got %r and %r"
                             % (min_lesion_voxels, penalty))
        tol, tau = self._tolerances("lesionwise", nsd_tolerances)
        nb, d0, d1, d2 = (int(s) for s in pred_bits.shape)
        R, dev = int(R), pred_bits.device
        workspace = "cwf_lesionwise_ex_workspace" if tol else "cwf_lesionwise_workspace"
        nbytes = getattr(self.lib, workspace)(nb, R, d0, d1, d2)
        if nbytes < 0:
            raise _lib.CwfError("%s failed with status %d (B=%d R=%d %dx%dx%d)" % (workspace, nbytes, nb, R, d0, d1, d2))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        summary = torch.zeros((nb, R, 2), dtype=torch.float64, device=dev)
        counts = torch.zeros((nb, R, 6), dtype=torch.int64, device=dev)
        overflow = torch.zeros((nb, R), dtype=torch.int32, device=dev)
        table = torch.zeros((nb, R, 64, 4), dtype=torch.int64, device=dev)
        lesion_hd95 = torch.zeros((nb, R, 64), dtype=torch.float64, device=dev)
        if tol:
            lesion_nsd = torch.zeros((nb, R, 64, len(tol)), dtype=torch.float64, device=dev)
            lw_nsd = torch.zeros((nb, R, len(tol)), dtype=torch.float64, device=dev)
            self._call("cwf_lesionwise_ex", pred_bits.data_ptr(), gt_bits.data_ptr(), nb, R, d0, d1, d2, int(dilation),
                       int(min_lesion_voxels), float(penalty), tau, len(tol), summary.data_ptr(), counts.data_ptr(), overflow.data_ptr(),
                       table.data_ptr(), lesion_hd95.data_ptr(), lesion_nsd.data_ptr(), lw_nsd.data_ptr(), ws.data_ptr(), int(nbytes),
                       self._stream())
            return summary, counts, overflow, table, lesion_hd95, lesion_nsd, lw_nsd
        self._call("cwf_lesionwise", pred_bits.data_ptr(), gt_bits.data_ptr(), nb, R, d0, d1, d2, int(dilation), int(min_lesion_voxels),
                   float(penalty), summary.data_ptr(), counts.data_ptr(), overflow.data_ptr(), table.data_ptr(), lesion_hd95.data_ptr(),
                   ws.data_ptr(), int(nbytes), self._stream())
        return summary, counts, overflow, table, lesion_hd95

    # ------------------------------------------------------------------ N5 sliding-window inference over volumes of any size
    @staticmethod
    def window_grid(nb, shape, roi, starts):
        """struct cwf_window_grid for nb samples of a volume `shape` (S0, S1, S2), windows `roi` (r0, r1, r2) at the per-axis `starts`
        (three lists; window w = (i0 * n1 + i1) * n2 + i2).  The kernels check the grid; this only packs it."""
        g = _lib.WindowGrid()
        g.B = int(nb)
        for a in range(3):
            g.S[a], g.r[a], g.n[a] = int(shape[a]), int(roi[a]), len(starts[a])
            if len(starts[a]) > _lib.WINDOW_MAX_STARTS:
                raise ValueError("window grid: %d windows along axis %d, at most %d" % (len(starts[a]), a, _lib.WINDOW_MAX_STARTS))
            for i, s in enumerate(starts[a]):
                g.start[a][i] = int(s)
        return g

    def window_gather(self, x, grid, w0, count):
        """x [B,4,S0,S1,S2] fp32 (made contiguous) -> windows w0 .. w0+count-1 of `grid` (window_grid), logical NCDHW
        [count*B,4,r0,r1,r2] over channels-last memory (sample j*B + b = window w0+j of sample b), zeros outside the volume
        (cwf_window_gather).  The model's permute(0,2,3,4,1).contiguous() of it copies nothing."""
        x = x.contiguous()
        assert x.dtype == _f32 and x.dim() == 5 and x.shape[1] == 4
        r = tuple(grid.r)
        win = torch.empty((int(count) * grid.B,) + r + (4,), dtype=_f32, device=x.device)
        self._call("cwf_window_gather", x.data_ptr(), win.data_ptr(), ctypes.byref(grid), int(w0), int(count), self._stream())
        return win.permute(0, 4, 1, 2, 3)

    def window_blend(self, probs, weights, acc, grid, w0, count, accumulate):
        """acc [B,S0,S1,S2,4] fp32 += the importance-weighted probabilities of windows w0 .. w0+count-1 (accumulate=False: the first
        chunk, acc is overwritten).  probs: the model's [count*B,4,r0,r1,r2] output; a view that is not channels-last contiguous is
        made one.  weights: the 1-D tables g0 | g1 | g2, fp32 [r0+r1+r2] on the device (cwf_window_blend)."""
        p = probs.permute(0, 2, 3, 4, 1)
        if not p.is_contiguous():
            p = p.contiguous()
        r = tuple(grid.r)
        assert p.dtype == _f32 and tuple(p.shape) == (int(count) * grid.B,) + r + (4,), (tuple(probs.shape), r, count)
        assert acc.is_contiguous() and tuple(acc.shape) == (grid.B,) + tuple(grid.S) + (4,)
        assert weights.is_contiguous() and weights.dtype == _f32 and weights.numel() == sum(r)
        self._call("cwf_window_blend", p.data_ptr(), weights.data_ptr(), acc.data_ptr(), ctypes.byref(grid), int(w0), int(count),
                   int(bool(accumulate)), self._stream())
        return acc

    def window_finalize(self, acc, weights, grid):
        """acc [B,S0,S1,S2,4] / per-voxel weight sum -> prob [B,4,S0,S1,S2] NCDHW (cwf_window_finalize)"""
        assert acc.is_contiguous() and tuple(acc.shape) == (grid.B,) + tuple(grid.S) + (4,)
        assert weights.is_contiguous() and weights.dtype == _f32 and weights.numel() == sum(grid.r)
        y = torch.empty((grid.B, 4) + tuple(grid.S), dtype=_f32, device=acc.device)
        self._call("cwf_window_finalize", acc.data_ptr(), weights.data_ptr(), y.data_ptr(), ctypes.byref(grid), self._stream())
        return y

    @staticmethod
    def window_box(full, lo):
        """struct cwf_window_box: the grid's volume is the box [lo, lo + grid.S) of a volume of extent `full`.  Only packs it."""
        bx = _lib.WindowBox()
        for a in range(3):
            bx.full[a], bx.lo[a] = int(full[a]), int(lo[a])
        return bx

    def window_gather_box(self, x, grid, box, w0, count):
        """window_gather of the crop x[:, :, lo0:lo0+S0, lo1:lo1+S1, lo2:lo2+S2] (S = grid.S, lo = box.lo), bit for bit, reading the
        whole x [B,4,*box.full] in place: voxels of a window outside the box are zero (cwf_window_gather_box)."""
        x = x.contiguous()
        assert x.dtype == _f32 and x.dim() == 5 and x.shape[1] == 4 and tuple(x.shape[2:]) == tuple(box.full) and x.shape[0] == grid.B
        r = tuple(grid.r)
        win = torch.empty((int(count) * grid.B,) + r + (4,), dtype=_f32, device=x.device)
        self._call("cwf_window_gather_box", x.data_ptr(), win.data_ptr(), ctypes.byref(grid), ctypes.byref(box), int(w0), int(count),
                   self._stream())
        return win.permute(0, 4, 1, 2, 3)

    def window_finalize_box(self, acc, weights, grid, box, out=None):
        """acc [B,S0,S1,S2,4] in box coordinates -> prob [B,4,*box.full] NCDHW: window_finalize's values inside the box, the background
        one-hot (1, 0, 0, 0) outside it, every element written once by one launch (cwf_window_finalize_box).  out: the tensor to fill."""
        assert acc.is_contiguous() and tuple(acc.shape) == (grid.B,) + tuple(grid.S) + (4,)
        assert weights.is_contiguous() and weights.dtype == _f32 and weights.numel() == sum(grid.r)
        shape = (grid.B, 4) + tuple(box.full)
        y = torch.empty(shape, dtype=_f32, device=acc.device) if out is None else out
        assert y.is_contiguous() and y.dtype == _f32 and tuple(y.shape) == shape and y.device == acc.device
        self._call("cwf_window_finalize_box", acc.data_ptr(), weights.data_ptr(), y.data_ptr(), ctypes.byref(grid), ctypes.byref(box),
                   self._stream())
        return y

    # ------------------------------------------------------------------ N3 training-batch preparation
    def prepare_batch(self, images, labels, params, crop, out=None):
        """Training batch (x [B,4,C0,C1,C2] fp32, target [B,C0,C1,C2] int64, edge [B,C0,C1,C2] int64) from per-sample source volumes
        (images[b] fp32 [4,S0,S1,S2], labels[b] uint8 [S0,S1,S2], contiguous, one device) in launches of eight samples (cwf_prepare_batch).
        params[b]: .origin (3 ints), .flip (3 bools), .scale / .shift (4 floats each, or None: intensity off), .matrix (9 floats, or
        None).  When some sample has a matrix the batch goes through cwf_prepare_batch_affine (rotated / zoomed crops, any origin), the
        samples without one with the identity.  .disp (float32 [3, G0, G1, G2] control grid, or None): when some sample has one the
        batch goes through cwf_prepare_batch_elastic, the samples without one with disp = NULL.  The grids of the call are packed into
        one pinned host buffer and copied to the device by one non-blocking copy on the current stream ahead of the launches (no host
        synchronisation; both buffers are handed back to torch's stream-ordered allocators once the launches are enqueued).  out:
        (x, target, edge) to write into; each needs contiguous inner dimensions, its sample stride may be larger than one sample.
        .blur / .noise / .noise_key / .gamma (utils.data.AugParams): when some channel of some sample has one on, the intensity stage
        (cwf_augment_intensity) follows on x: in place without a blur; with one the prepare kernel writes x into a workspace from
        torch's allocator and the stage writes the batch's x.  With all of them off nothing but the prepare entry is called.
        .bias / .bias_mask / .contrast / .lowres: when some channel of some sample has one on, the acquisition stage
        (cwf_augment_acquisition) runs between the two: in place on what the prepare kernel wrote without a lowres bit; with one
        it gathers into the next buffer of the chain (the batch's x, or a second workspace when a blur follows).  The control
        multipliers travel as the elastic grids do.  At most two batch-sized workspaces, from torch's allocator, which hands the
        same blocks out again call after call."""
        crop = tuple(int(c) for c in crop)
        if len(crop) != 3:
            raise ValueError("prepare_batch: crop needs three extents, got %r" % (crop,))
        nb = len(images)
        if len(labels) != nb or len(params) != nb:
            raise ValueError("prepare_batch: %d images, %d labels and %d parameter sets" % (nb, len(labels), len(params)))
        if nb == 0:
            raise ValueError("prepare_batch: empty batch")
        dev = images[0].device
        if dev.type != "cuda":
            raise ValueError("prepare_batch: the images must be on a GPU")
        grids = [getattr(p, "disp", None) for p in params]
        elastic = any(g is not None for g in grids)
        affine = elastic or any(getattr(p, "matrix", None) is not None for p in params)
        samples = ((_lib.PrepElasticSample if elastic else _lib.PrepAffineSample if affine else _lib.PrepSample) * nb)()
        entry = "cwf_prepare_batch_elastic" if elastic else "cwf_prepare_batch_affine" if affine else "cwf_prepare_batch"
        disp_dev = None
        if elastic:
            sizes = [0 if g is None else int(g.size) for g in grids]
            host = torch.empty(sum(sizes), dtype=_f32, pin_memory=True)
            view, at = host.numpy(), 0
            for g, n in zip(grids, sizes):
                if g is not None:
                    if g.dtype != np.float32 or g.ndim != 4 or g.shape[0] != 3:
                        raise ValueError("prepare_batch: disp must be a float32 [3, G0, G1, G2] array, got %s %r" % (g.dtype, g.shape))
                    view[at:at + n] = g.reshape(-1)
                    at += n
            disp_dev = torch.empty(host.numel(), dtype=_f32, device=dev)
            disp_dev.copy_(host, non_blocking=True)
        for b, (img, lab, p) in enumerate(zip(images, labels, params)):
            if img.dtype != _f32 or img.dim() != 4 or img.shape[0] != 4 or not img.is_contiguous() or img.device != dev:
                raise ValueError("prepare_batch: images[%d] must be a contiguous float32 [4, S0, S1, S2] tensor on %s" % (b, dev))
            if lab.dtype != torch.uint8 or tuple(lab.shape) != tuple(img.shape[1:]) or not lab.is_contiguous() or lab.device != dev:
                raise ValueError("prepare_batch: labels[%d] must be a contiguous uint8 %s tensor on %s" % (b, tuple(img.shape[1:]), dev))
            s = samples[b]
            s.image, s.label = img.data_ptr(), lab.data_ptr()
            s.S0, s.S1, s.S2 = (int(v) for v in img.shape[1:])
            s.o0, s.o1, s.o2 = (int(v) for v in p.origin)
            s.flip = sum(1 << i for i, f in enumerate(p.flip) if f)
            s.intensity = int(p.scale is not None)
            if p.scale is not None:
                s.scale[:] = [float(v) for v in p.scale]
                s.shift[:] = [float(v) for v in p.shift]
            if affine:
                m = getattr(p, "matrix", None)
                s.m[:] = [float(v) for v in m] if m is not None else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
            if elastic and grids[b] is not None:
                s.disp = disp_dev.data_ptr() + 4 * sum(sizes[:b])
                s.G0, s.G1, s.G2 = (int(v) for v in grids[b].shape[1:])
        if out is None:
            # (a crop the library refuses -- an extent <= 0 or 2^31 voxels and more -- gets placeholders: the refusal comes from it)
            ok = all(c > 0 for c in crop) and crop[0] * crop[1] * crop[2] < (1 << 31)
            shape = crop if ok else (1, 1, 1)
            x = torch.empty((nb, 4) + shape, dtype=_f32, device=dev)
            target = torch.empty((nb,) + shape, dtype=torch.int64, device=dev)
            edge = torch.empty((nb,) + shape, dtype=torch.int64, device=dev)
        else:
            x, target, edge = out
            for name, t, shape, dt in (("x", x, (nb, 4) + crop, _f32), ("target", target, (nb,) + crop, torch.int64),
                                       ("edge", edge, (nb,) + crop, torch.int64)):
                inner = torch.empty(shape[1:], device="meta").stride()
                if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or tuple(t.stride()[1:]) != inner:
                    raise ValueError("prepare_batch: out %s must be a %s %s tensor on %s with contiguous samples" % (name, dt, shape, dev))
        stage = self._intensity_samples(params)
        acq, bias_dev = self._acquire_samples(params, crop, dev)
        blur = stage is not None and any(s.blur for s in stage)   # a blur reads its neighbours: not in place
        lowres = acq is not None and any(s.lowres_mask for s in acq)    # nor does the gather of the low-resolution step

        def scratch():
            return torch.empty((nb, 4) + tuple(x.shape[2:]), dtype=_f32, device=dev)

        x_acq = scratch() if blur else x                          # what the intensity stage reads
        x_prep = scratch() if lowres else x_acq                   # what the prepare kernel writes
        self._call(entry, ctypes.addressof(samples), nb, crop[0], crop[1], crop[2], x_prep.data_ptr(), x_prep.stride(0),
                   target.data_ptr(), target.stride(0), edge.data_ptr(), edge.stride(0), self._stream())
        if acq is not None:
            nws = _lib.acquire_ws_doubles(nb, crop) if any(s.contrast_mask for s in acq) else 0
            ws = torch.empty(nws, dtype=torch.float64, device=dev) if nws else None
            self._call("cwf_augment_acquisition", ctypes.addressof(acq), nb, crop[0], crop[1], crop[2], x_prep.data_ptr(),
                       x_prep.stride(0), x_acq.data_ptr(), x_acq.stride(0), _p(ws), nws, self._stream())
        x_prep = x_acq
        if stage is not None:
            nws = _lib.intensity_ws_floats(nb, crop) if any(s.gam for s in stage) else 0
            ws = torch.empty(nws, dtype=_f32, device=dev) if nws else None
            self._call("cwf_augment_intensity", ctypes.addressof(stage), nb, crop[0], crop[1], crop[2], x_prep.data_ptr(),
                       x_prep.stride(0), x.data_ptr(), x.stride(0), _p(ws), nws, self._stream())
        return x, target, edge

    @staticmethod
    def _acquire_samples(params, crop, dev):
        """(cwf_acquire_sample [len(params)], the device tensor that holds their control multipliers or None) of the samples' bias /
        contrast / lowres, or (None, None) when every channel of every one is off.  The grids of the channels that are on are packed
        into one pinned host buffer and copied by one non-blocking copy on the current stream."""
        from utils import data
        acq = (_lib.AcquireSample * len(params))()
        on, grids = False, []
        for s, p in zip(acq, params):
            mask, bias = getattr(p, "bias_mask", None), getattr(p, "bias", None)
            contrast, lowres = getattr(p, "contrast", None), getattr(p, "lowres", None)
            if bias is not None and mask is not None and any(mask):
                if bias.dtype != np.float32 or bias.ndim != 4 or bias.shape[0] != 4:
                    raise ValueError("prepare_batch: bias must be a float32 [4, G0, G1, G2] array, got %s %r" % (bias.dtype, bias.shape))
                s.G0, s.G1, s.G2 = (int(v) for v in bias.shape[1:])
            for c in range(4):
                if bias is not None and mask is not None and mask[c]:
                    grids.append((s, c, bias[c]))
                    s.bias_mask |= 1 << c
                if contrast is not None and contrast[c] > 0.0:
                    s.factor[c] = float(contrast[c])
                    s.contrast_mask |= 1 << c
                if lowres is not None and lowres[c] > 0.0:
                    s.lattice[c][:] = data.lowres_lattice(crop, lowres[c])
                    s.lowres_mask |= 1 << c
            on = on or bool(s.bias_mask or s.contrast_mask or s.lowres_mask)
        if not on:
            return None, None
        bias_dev = None
        if grids:
            host = torch.empty(sum(int(g.size) for _, _, g in grids), dtype=_f32, pin_memory=True)
            view, at = host.numpy(), 0
            bias_dev = torch.empty(host.numel(), dtype=_f32, device=dev)
            for s, c, g in grids:
                view[at:at + g.size] = g.reshape(-1)
                s.bias[c] = bias_dev.data_ptr() + 4 * at
                at += int(g.size)
            bias_dev.copy_(host, non_blocking=True)
        return acq, bias_dev

    @staticmethod
    def _intensity_samples(params):
        """cwf_intensity_sample [len(params)] of the samples' blur / noise / gamma, or None when every channel of every one is off"""
        from utils import data
        stage = (_lib.IntensitySample * len(params))()
        on = False
        for s, p in zip(stage, params):
            blur, noise, gamma = (getattr(p, k, None) for k in ("blur", "noise", "gamma"))
            s.key = int(getattr(p, "noise_key", 0) or 0)
            for c in range(4):
                if blur is not None and blur[c] > 0.0:
                    s.taps[c][:] = data.blur_taps64(blur[c])              # (ctypes rounds to float32, to nearest)
                    s.blur |= 1 << c
                if noise is not None and noise[c] > 0.0:
                    s.amp[c] = data.noise_amp64(noise[c])
                    s.noise |= 1 << c
                if gamma is not None and gamma[c] > 0.0:
                    s.gamma[c] = float(gamma[c])
                    s.gam |= 1 << c
            on = on or bool(s.blur or s.noise or s.gam)
        return stage if on else None

    def normalize_nonzero(self, image):
        """In place: per-channel z-score of one subject image (contiguous fp32 [4, H, W, D] on a GPU) over the voxels whose
        four-channel sum is > 0, float64 two-pass statistics (cwf_normalize_nonzero).  Returns image."""
        if image.dtype != _f32 or image.dim() != 4 or image.shape[0] != 4 or not image.is_contiguous() or not image.is_cuda:
            raise ValueError("normalize_nonzero: image must be a contiguous float32 [4, H, W, D] tensor on a GPU")
        ws = torch.empty(_lib.NORM_WS_DOUBLES, dtype=torch.float64, device=image.device)
        self._call("cwf_normalize_nonzero", image.data_ptr(), image[0].numel(), ws.data_ptr(), self._stream())
        return image

    def class_locations(self, label, posmasks, K, out=None):
        """label: a contiguous uint8 tensor on a GPU (any shape; its C-order linear index is what the table holds) -> (counts int64
        [R], table int32 [R, K]) on its device: per region (class bitmask over classes 0..3, label 4 read as 3) the voxel count and
        the evenly ranked table of linear indices, -1 past min(count, K) (cwf_class_locations).  out: (counts, table) to write into,
        e.g. one subject's rows of a [n, R] / [n, R, K] pair.  No host synchronisation."""
        if label.dtype != torch.uint8 or not label.is_cuda or not label.is_contiguous() or label.numel() < 1:
            raise ValueError("class_locations: label must be a non-empty contiguous uint8 tensor on a GPU")
        masks, cm = self._posmasks("class_locations", posmasks)
        R, K, V = len(masks), int(K), int(label.numel())
        nbytes = self.lib.cwf_class_locations_workspace(V, R)
        if nbytes < 0:
            raise _lib.CwfError("cwf_class_locations_workspace failed with status %d (V=%d R=%d)" % (nbytes, V, R))
        if out is None:
            if not 1 <= K <= 65536:
                raise _lib.CwfError("cwf_class_locations: K must lie in 1..65536, got %d" % K)
            out = (torch.empty(R, dtype=torch.int64, device=label.device), torch.empty((R, K), dtype=torch.int32, device=label.device))
        counts, table = out
        if counts.dtype != torch.int64 or tuple(counts.shape) != (R,) or table.dtype != torch.int32 or tuple(table.shape) != (R, K) \
                or not counts.is_contiguous() or not table.is_contiguous() or counts.device != label.device or table.device != label.device:
            raise ValueError("class_locations: out must be contiguous (int64 [%d], int32 [%d, %d]) tensors on the label's device" % (R, R, K))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=label.device)
        self._call("cwf_class_locations", label.data_ptr(), V, ctypes.addressof(cm), R, K, counts.data_ptr(), table.data_ptr(),
                   ws.data_ptr(), self._stream())
        return counts, table

    def nonzero_box(self, x, out=None):
        """x fp32 [B,4,S0,S1,S2] on a GPU, each sample's four channels contiguous (a batch stride of its own is fine, any 4-byte
        alignment) -> (box int32 [B,6] = lo0, lo1, lo2, hi0, hi1, hi2 with hi exclusive, count int64 [B]) on its device: the tightest
        box of the voxels with a channel whose bits & 0x7fffffff != 0, and their number; lo = S, hi = 0, count = 0 for a sample
        without one (cwf_nonzero_box).  out: (box, count) to write into, e.g. one subject's rows.  No host synchronisation."""
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == _f32 and x.dim() == 5 and x.shape[1] == 4 and x.numel() > 0):
            raise ValueError("nonzero_box: x must be a non-empty float32 [B, 4, S0, S1, S2] tensor on a GPU")
        if not x[0].is_contiguous() or (x.shape[0] > 1 and x.stride(0) < x[0].numel()):
            x = x.contiguous()
        B, (S0, S1, S2) = int(x.shape[0]), (int(s) for s in x.shape[2:])
        nbytes = self.lib.cwf_nonzero_box_workspace(B, S0, S1, S2)
        if nbytes < 0:
            raise _lib.CwfError("cwf_nonzero_box_workspace failed with status %d (B=%d S=%r)" % (nbytes, B, (S0, S1, S2)))
        if out is None:
            out = (torch.empty((B, 6), dtype=torch.int32, device=x.device), torch.empty(B, dtype=torch.int64, device=x.device))
        box, count = out
        if box.dtype != torch.int32 or tuple(box.shape) != (B, 6) or count.dtype != torch.int64 or tuple(count.shape) != (B,) \
                or not box.is_contiguous() or not count.is_contiguous() or box.device != x.device or count.device != x.device:
            raise ValueError("nonzero_box: out must be contiguous (int32 [%d, 6], int64 [%d]) tensors on x's device" % (B, B))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)
        bstride = int(x.stride(0)) if B > 1 else 4 * S0 * S1 * S2
        self._call("cwf_nonzero_box", x.data_ptr(), bstride, B, S0, S1, S2, box.data_ptr(), count.data_ptr(), ws.data_ptr(),
                   self._stream())
        return box, count

    # ------------------------------------------------------------------ K11 / misc
    def adam(self, table, ntensors, max_n, lr, beta1, beta2, eps, wd, step, amsgrad, hyper_dev=None, grad_scale=1.0):
        self._call("cwf_adam_amsgrad_scaled", table.data_ptr(), ntensors, max_n, lr, beta1, beta2, eps, wd, step, int(amsgrad),
                   _p(hyper_dev), float(grad_scale), self._stream())

    # ------------------------------------------------------------------ K13 step controls (csrc/grad_step.hip)
    @staticmethod
    def _flat_f32(name, t):
        if t.dtype != _f32 or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("%s: a contiguous 1-D float32 tensor on a GPU is required" % name)

    def grad_add(self, a, b, y):
        """y = a + b on flat float32 slices (b None: y = a); y may be a or b.  Returns y."""
        for t in (a, y) + (() if b is None else (b,)):
            self._flat_f32("grad_add", t)
            if t.numel() != y.numel():
                raise ValueError("grad_add: operands differ in length")
        self._call("cwf_grad_add", a.data_ptr(), _p(b), y.data_ptr(), y.numel(), self._stream())
        return y

    def grad_norm_clip(self, g, grad_scale, max_norm, ws, out2):
        """out2 = {grad_scale * min(1, max_norm / (norm + 1e-6)), norm}, norm = grad_scale * |g|_2 with a double sum; nothing is
        read back.  ws: float64 [GRADNORM_WS_DOUBLES] scratch (holds the per-workgroup partial sums afterwards)."""
        self._flat_f32("grad_norm_clip", g)
        self._flat_f32("grad_norm_clip", out2)
        if out2.numel() != 2 or ws.dtype != torch.float64 or ws.numel() < _lib.GRADNORM_WS_DOUBLES or not ws.is_contiguous() \
                or ws.device != g.device or out2.device != g.device:
            raise ValueError("grad_norm_clip: out2 must be float32 [2] and ws float64 [%d] on g's device" % _lib.GRADNORM_WS_DOUBLES)
        self._call("cwf_grad_norm_clip", g.data_ptr(), g.numel(), float(grad_scale), float(max_norm), ws.data_ptr(), out2.data_ptr(),
                   self._stream())
        return out2

    def adam_ex(self, table, ntensors, max_n, lr, beta1, beta2, eps, wd, step, amsgrad, hyper_dev=None, grad_scale=1.0,
                gscale_dev=None, ema_table=None, ema_weight=0.0):
        """adam() with the gradient scale read from the device (gscale_dev: float32 [>= 1]) and / or an EMA of the new weights
        (ema_table: int64 [ntensors] of device addresses parallel to table, ema_weight = 1 - decay)."""
        if ema_table is not None and (ema_table.dtype != torch.int64 or ema_table.numel() != ntensors or not ema_table.is_cuda):
            raise ValueError("adam_ex: ema_table must hold one int64 device address per tensor, on the GPU")
        self._call("cwf_adam_amsgrad_ex", table.data_ptr(), ntensors, max_n, lr, beta1, beta2, eps, wd, step, int(amsgrad),
                   _p(hyper_dev), float(grad_scale), _p(gscale_dev), _p(ema_table), float(ema_weight), self._stream())

    # ------------------------------------------------------------------ K14 AdamW / SGD rules (csrc/optim_rules.hip)
    def optim_step(self, rule, table, ntensors, max_n, lr, wd, wd_mul=None, beta1=0.9, beta2=0.999, eps=1e-8, step=0, amsgrad=False,
                   hyper_dev=None, momentum=0.0, dampening=0.0, nesterov=False, first=False, grad_scale=1.0, gscale_dev=None,
                   ema_table=None, ema_weight=0.0):
        """One launch of rule "adamw" (torch.optim.AdamW) or "sgd" (torch.optim.SGD; the momentum buffer is the table's exp_avg
        column, `first`: this is the buffers' first update) over a descriptor table.  wd_mul: float32 [ntensors] on the GPU, the
        per-tensor multiplier of wd (None: all ones); gscale_dev / ema_table / ema_weight as in adam_ex."""
        rules = {"adamw": _lib.RULE_ADAMW, "sgd": _lib.RULE_SGD}
        if rule not in rules:
            raise ValueError("optim_step: rule must be 'adamw' or 'sgd', got %r" % (rule,))
        if wd_mul is not None and (wd_mul.dtype != _f32 or wd_mul.numel() != ntensors or not wd_mul.is_cuda or not wd_mul.is_contiguous()):
            raise ValueError("optim_step: wd_mul must hold one float32 per tensor, on the GPU")
        if ema_table is not None and (ema_table.dtype != torch.int64 or ema_table.numel() != ntensors or not ema_table.is_cuda):
            raise ValueError("optim_step: ema_table must hold one int64 device address per tensor, on the GPU")
        self._call("cwf_optim_step", rules[rule], table.data_ptr(), ntensors, max_n, float(lr), float(wd), _p(wd_mul), float(beta1),
                   float(beta2), float(eps), int(step), int(amsgrad), _p(hyper_dev), float(momentum), float(dampening), int(nesterov),
                   int(first), float(grad_scale), _p(gscale_dev), _p(ema_table), float(ema_weight), self._stream())

    def dropout_mask(self, shape, p, device, p2=0.0):
        """Pre-scaled keep mask(s) in one launch from the device generator state (capturable: the state advances by a kernel)."""
        m = torch.empty(shape, dtype=_f32, device=device)
        n = m.numel()
        self._call("cwf_dropout_mask_rng", m.data_ptr(), n, float(p), float(p2), self.rng(device).data_ptr(), self.rng_site(n), self._stream())
        return m

    def mul(self, a, b):
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        self._call("cwf_mul", a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), self._stream())
        return y

    def add(self, a, b):
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        self._call("cwf_add", a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), self._stream())
        return y

    def channel_scale(self, x, s):
        x, ldc = cl(x)
        n, d, h, w, c = x.shape
        y = torch.empty((n, d, h, w, c), dtype=_f32, device=x.device)
        self._call("cwf_channel_scale", x.data_ptr(), ldc, s.data_ptr(), y.data_ptr(), c, n, d * h * w, c, self._stream())
        return y

    def copy_into(self, x, out):
        """out[..., :] = x for channels-last views (zero-copy concat helper)."""
        x, ldc = cl(x)
        n, d, h, w, c = x.shape
        self._call("cwf_copy_strided", x.data_ptr(), ldc, out.data_ptr(), out.stride(3), n * d * h * w, c, self._stream())
        return out


_backend = None


def backend():
    """The kernel backend of the product path: always the HIP library."""
    global _backend
    if _backend is None:
        _backend = HipBackend()
    return _backend


def _set_backend_for_testing(obj):
    """TEST-ONLY hook (tests/ inject oracle/kernel_emul.py to exercise the host-side autograd wiring on CPU).
    Nothing in the package calls this."""
    global _backend
    _backend = obj
