"""Training-step harness: the reference hot loop (train_no_amp.py:181-239) without its per-iteration host syncs.

    forward -> softmax_dice + 2x get_separate_loss + 2x get_edge_separate_loss (all weights 1.0, :205-211)
    -> backward -> gradient average over ranks -> Adam(amsgrad) with the poly learning rate (:183,270-273).

Execution modes:
  * eager (default): every kernel is launched from Python (~460 launches, ~16-21 ms of host time per step, hidden behind the GPU's
    ~23 ms); the three sub-regions share each launch (grouped kernels), weight gradients run on a side stream.
  * plan (use_graph=True or "plan"): forward + losses + backward + gradient reduces are captured ONCE (stream capture through
    torch.cuda.graph; shapes are static -- fixed patch size, per-sample top-k of fixed k -- and the token selection and the dropout
    counters live on device, so nothing in the step needs the host) and re-issued per step by the library as a plain LAUNCH LIST
    (csrc/plan.hip: one hipModuleLaunchKernel per node on the capture's stream chains, events for the cross-stream edges; ONE
    Python -> C call per step, or one per gradient phase when data-parallel).  Host cost ~2 ms per step instead of ~16.
  * hipgraph (use_graph="hipgraph"): the same capture replayed with hipGraphLaunch -- slower end to end than eager on this ROCm
    build (~44 us of host time per node); only on request.  A capture the plan cannot express (a copy node) is
    dropped and the Trainer goes on with eager steps.
Gradients never exist as per-parameter tensors: backward kernels write them into ONE flat buffer laid out in backward-completion
order (cwf.optim.GradSink; the conv weight gradients through one batched split-K reduce per phase), which the fused Adam launch reads.
Multi-GPU gradient averaging (the only data-path collective) is overlapped with backward: the model fires a callback when backward
has passed a cut point (decoder done / everything but the encoder done, ClsWiseFormer.grad_phases); the phase's contiguous slice
(9.8 MB, then 43 MB) is all-reduced (RCCL, summed; Adam reads g / world) on a communication stream that waits for the producing
streams -- the three region streams and the weight-gradient side stream stay in use -- while the encoder's backward (~7 ms) runs;
only the last 14 MB slice is exposed.  In plan mode the cut points are captured as marker nodes on the communication stream; the
launch list is issued up to a marker, the phase's all-reduce is enqueued behind it, and the list continues.  Under hipGraph replay
the collective follows the replay (4 chunks of the flat buffer).
CWF_FORCE_COMM=1 keeps the whole collective path on at world size 1 (a one-rank RCCL group): the way to exercise and profile it on a
one-GPU box.
Step controls (all off by default; then the step issues exactly the launches described above):
  * accum_steps = N: step() is called once per micro-batch; micro-steps 1..N-1 run forward and backward, issue NO collective and
    add the flat gradient to the optimizer's accumulator (one launch on the main stream, after the weight-gradient stream has been
    joined); micro-step N adds the accumulator to the flat buffer -- per phase slice on the communication stream just before that
    slice's all-reduce when communication is overlapped, else in one launch after backward -- and updates with the gradient
    1/(world N) sum_ranks sum_micro g: N independent forwards whose gradients are averaged, the reference's only batch semantics
    (SURVEY.md F2).  Accumulate and fold launches are never captured: the captured step is the same for every micro-step.
  * max_grad_norm: the averaged gradient is clipped by its global norm inside the Adam launch (cwf.optim); no host sync.
  * ema_decay: the Adam launch also maintains an EMA copy of the weights (ema_state_dict() for validation / checkpoints).
  * <name>_weight = w for a supplementary loss term of cwf.loss_terms.TERMS: w * the term of the main output (outputs[0]) becomes a
    further part, appended after the reference's five in the table's order and added to the total in front of the same backward.  w
    lives in a one-float device tensor that the kernels read, made at the first step that needs it (before a capture), so
    set_<name>_weight() between steps needs no recapture; the term's other options are launch arguments, fixed at construction.
    None: the step makes no new call and total_loss is called without that keyword, as before the term existed.
      boundary: tools.boundary_loss, signed distance maps of the target's WT / TC / ET computed on the device every step.
      topk (topk_percent = K): tools.topk_ce, mean of -log p_target over the hardest K % of the batch's voxels, selected exactly.
      focal (focal_params = {...}): tools.focal_loss, focal Tversky on WT / TC / ET + ce_ratio * focal cross-entropy, batch sums.
      lovasz (lovasz_regions = "classes" | "regions" | class bitmasks, lovasz_only_present): tools.lovasz_softmax, exact sort.
    A new term is one entry of that table, its pair of backend methods (cwf.kernels, cwf.functional) and its utils.tools wrapper.
  * optimizer = "adamw" | "sgd" (with betas / momentum, nesterov / no_decay): the update is one launch of the AdamW or SGD rule
    (cwf.optim.FusedAdamW / FusedSGD) in place of Adam's; sink, all-reduce, accumulation, clipping and EMA are the base class's and
    work as above.  schedule = "cosine" | "constant" and warmup_steps = W shape the learning rate of an update:
    schedule(init_lr, epoch, end_epoch) * min(1, (updates_done + 1) / W), updates_done counting weight updates.
Checkpoints use the reference layout {'epoch', 'state_dict' with 'module.' prefix, 'optim_dict'} (:248-253)."""
from __future__ import annotations

import functools
import os

import torch
import torch.distributed as dist

from . import loss_terms
from .optim import FusedAdam, FusedAdamW, FusedSGD, SCHEDULES, poly_lr, schedule_lr, warmup_factor


def total_loss(outputs, target, edge, boundary=None, topk=None, focal=None, lovasz=None):
    """The reference's five terms, then one part per supplementary term that is given (cwf.loss_terms.TERMS, whose order the
    keywords follow): tools.<tool>(outputs[0], target, ...) at the weight in the term's one-float device tensor, appended and added
    to the total.  `boundary` is that tensor; a term with options receives (the tensor, *its options): topk = (tensor, percent),
    focal = (tensor, the keyword arguments of tools.focal_loss), lovasz = (tensor, the region masks, only_present)."""
    from models import criterions
    from utils import tools
    parts = [criterions.softmax_dice(outputs[0], target), tools.get_separate_loss(outputs[1], target),
             tools.get_edge_separate_loss(outputs[2], edge), tools.get_separate_loss(outputs[3], target),
             tools.get_edge_separate_loss(outputs[4], edge)]
    total = parts[0] + parts[1] + parts[2] + parts[3] + parts[4]
    for term, value in zip(loss_terms.TERMS, (boundary, topk, focal, lovasz)):
        if value is not None:
            parts.append(getattr(tools, term.tool)(outputs[0], target, **loss_terms.unpack(term, value)))
            total = total + parts[-1]
    return total, parts


def check_boundary_weight(w):
    """None (term off) or a finite float >= 0"""
    return loss_terms.check_weight("boundary", w)


# (weight, *options as given) -> (weight, *options as the Trainer stores them), ValueError for a bad value: cwf.loss_terms.check
check_topk = functools.partial(loss_terms.check, "topk")            # (weight, percent)
check_focal = functools.partial(loss_terms.check, "focal")          # (weight, params) -> (weight, every keyword of tools.focal_loss)
check_lovasz = functools.partial(loss_terms.check, "lovasz")        # (weight, regions="classes", only_present=True) -> (weight, masks, ..)


def boundary_schedule(weight, epoch, warmup):
    """--boundary_weight A / --boundary_warmup E: A * min(1, epoch / E), E = 0 meaning constant"""
    return float(weight) if warmup <= 0 else float(weight) * min(1.0, float(epoch) / float(warmup))


def kernels_backend():
    from .kernels import backend
    return backend()


class Trainer:
    def __init__(self, model, lr=2e-4, weight_decay=1e-5, amsgrad=True, end_epoch=1000, use_graph=False,
                 graph_warmup=2, overlap_comm=True, wgrad_async=True, accum_steps=1, max_grad_norm=None, ema_decay=None,
                 boundary_weight=None, topk_weight=None, topk_percent=10.0, optimizer="adam", betas=(0.9, 0.999), momentum=0.0,
                 nesterov=False, no_decay=None, schedule="poly", warmup_steps=0, focal_weight=None, focal_params=None,
                 lovasz_weight=None, lovasz_regions="classes", lovasz_only_present=True):
        given = locals()                                # (the keyword arguments by name; nothing else is bound yet)
        for term in loss_terms.TERMS:
            # a term's state, under the names its keywords have: <name>_weight (None: off), its options as cwf.loss_terms stores
            # them, and _<name>, the weight as a one-float device tensor, made at the first step that needs it
            keys = (term.name + "_weight",) + term.options
            for key, value in zip(keys, loss_terms.check(term.name, *(given[k] for k in keys))):
                setattr(self, key, value)
            setattr(self, "_" + term.name, None)
        self.model = model
        self.init_lr, self.end_epoch = lr, end_epoch
        if int(accum_steps) != accum_steps or accum_steps < 1:
            raise ValueError("accum_steps must be an integer >= 1")
        self.accum_steps = int(accum_steps)
        self._micro = 0                                 # micro-steps of the current window already accumulated
        self._last_micro = True                         # this call ends its window: fold, collectives, update
        phases = model.grad_phases() if hasattr(model, "grad_phases") else None
        if schedule not in SCHEDULES:
            raise ValueError("schedule must be one of %s, got %r" % (", ".join(SCHEDULES), schedule))
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError("warmup_steps must be an integer >= 0")
        self.schedule, self.warmup_steps = schedule, int(warmup_steps)
        controls = dict(phases=phases, max_grad_norm=max_grad_norm, ema_decay=ema_decay)
        if optimizer == "adam":
            if no_decay is not None:
                raise ValueError("optimizer='adam' decays every parameter: no_decay needs optimizer='adamw' or 'sgd'")
            self.opt = FusedAdam(model.parameters(), lr=lr, betas=betas, weight_decay=weight_decay, amsgrad=amsgrad, **controls)
        elif optimizer == "adamw":
            self.opt = FusedAdamW(model.named_parameters(), lr=lr, betas=betas, weight_decay=weight_decay, amsgrad=amsgrad,
                                  no_decay=no_decay, **controls)
        elif optimizer == "sgd":
            self.opt = FusedSGD(model.named_parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                                no_decay=no_decay, **controls)
        else:
            raise ValueError("optimizer must be 'adam', 'adamw' or 'sgd', got %r" % (optimizer,))
        self.optimizer = optimizer
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # collectives on: more than one rank, or a one-rank group with CWF_FORCE_COMM=1 (exercises the RCCL path on a one-GPU box)
        self.comm = self.world > 1 or (dist.is_available() and dist.is_initialized() and os.environ.get("CWF_FORCE_COMM", "0") == "1")
        # the all-reduce SUMS, the accumulator sums: Adam reads g / (world * micro-batches) (the DDP average, train_no_amp.py:133)
        self.opt.grad_scale = 1.0 / (self.world * self.accum_steps)
        if use_graph not in (False, True, None, "plan", "hipgraph"):
            raise ValueError("use_graph must be False, True, 'plan' or 'hipgraph'")
        self.graph_mode = {True: "plan", False: None, None: None}.get(use_graph, use_graph)
        self.use_graph = self.graph_mode is not None
        self.cuda = next(model.parameters()).is_cuda
        # weight gradients on a side stream (they are leaves of backward; the data-gradient chain is its critical path)
        self.wgrad_async = bool(wgrad_async) and self.cuda
        # all-reduce of a phase's slice as soon as backward has passed its cut point (eager; plan mode through captured markers)
        self.overlap_comm = bool(overlap_comm) and self.comm and self.graph_mode != "hipgraph"
        # HIGH priority: its own hardware-queue pool (a default-priority stream can land on the main stream's queue, see
        # cwf.kernels._priority_stream), and a collective should start the moment its slice is final
        self._comm_stream = (torch.cuda.Stream(priority=torch.cuda.Stream.priority_range()[1])
                             if (self.overlap_comm and self.cuda) else None)
        self._works = []
        if self.comm:
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, 0)
        if hasattr(model, "phase_callback"):
            model.phase_callback = self._phase_done
        self._graph = None
        self._plan = None
        self.plan_info = None
        self._static = None
        self._eager_steps = 0
        self._graph_warmup = graph_warmup
        self._in_backward = False
        # The decoder's (full-resolution) weight gradients are queued and released when backward leaves the decoder: they then run
        # beside the backward of the supervision heads / couplers -- 10-20 us kernels behind ~35 us of Python each, where the main
        # stream idles 1.7 ms per step -- instead of competing with the decoder's own HBM-bound data gradients (95.6 -> 96.7
        # volumes/s; neutral while the step was still bound elsewhere).  Holding the heads / couplers / decouplers phase's ~40 small
        # weight-gradient launches too, until backward is in the encoder, was best while the eight residual layers' weight gradients
        # still ran on the main stream (103.1 -> 104.8 volumes/s); with them on the side stream (functional.CarryLink) the SIDE
        # stream ends the step and must start earlier (launch plan, nothing / decoder / both held: 104.0 / 106.2 / 100.5).

    # ------------------------------------------------------------------------------------------------
    def _phase_done(self, k):
        """Backward has passed cut point k: every gradient of phase k has been produced (conv weight gradients as split-K slabs).
        Reduce the slabs of the layers seen so far into the flat buffer (one launch) and, data-parallel, start the all-reduce of
        the phase's contiguous slice on the communication stream while backward goes on."""
        if not self._in_backward:
            return
        K = kernels_backend()
        if K.wgrad_defer:
            # the decoder's weight gradients, queued during phase 0, start now: beside the GPU-light heads / couplers backward
            K.wgrad_release()
        K.wgrad_flush()
        if self.overlap_comm:
            self._allreduce_chunk(k)

    def _allreduce_chunk(self, k):
        lo, hi = self.opt.sink.chunks[k]
        if hi <= lo:
            return
        if not self._last_micro and not _capturing():
            return                                               # inside an accumulation window: no collective
        chunk = self.opt.flat_grad[lo:hi]
        if self._comm_stream is not None:
            K = kernels_backend()
            cs = self._comm_stream
            cs.wait_stream(torch.cuda.current_stream())          # coupler gradients (region streams are joined into this one by autograd)
            for st in K._wg_stream.values():
                cs.wait_stream(st)                               # the batched slab reduce of this phase
            with torch.cuda.stream(cs):
                if _capturing():
                    # plan mode: the cut point becomes a marker node behind both streams; the collective itself is enqueued on this
                    # stream by _run_plan when the launch list reaches the marker
                    K._call("cwf_plan_marker", int(k), K._stream())
                else:
                    if self._micro:
                        self.opt.fold(lo, hi)                    # the window's earlier micro-steps, before the collective reads the slice
                    self._works.append(dist.all_reduce(chunk, async_op=True))
        elif not _capturing():
            if self._micro:
                self.opt.fold(lo, hi)
            self._works.append(dist.all_reduce(chunk, async_op=True))

    def _fwd_bwd(self, x, target, edge):
        self.opt._ensure()
        sink = self.opt.sink
        sink.begin()
        K = kernels_backend()
        K.wgrad_async = self.wgrad_async       # (from the forward pass on: it prepares weight-gradient operands on the side stream)
        outputs = self.model(x, None)
        extra = {}                                      # (a term that is off is not named: total_loss is called as before it existed)
        for term in loss_terms.TERMS:
            wt = self._weight_tensor(term, x.device)
            if wt is not None:
                extra[term.name] = loss_terms.pack(term, wt, [getattr(self, k) for k in term.options])
        # (the first term's value travels fourth, positionally, None when off: wrappers written before the keywords take it so)
        loss, parts = total_loss(outputs, target, edge, extra.pop(loss_terms.TERMS[0].name, None), **extra)
        self.opt.zero_grad(set_to_none=True)
        # graph modes: one reduce per phase, in warm-up too
        K.flush_every = (1 << 30) if self.use_graph else K.flush_every_default
        K.wgrad_defer = self.wgrad_async and hasattr(self.model, "phase_callback")
        self._in_backward = True
        try:
            with sink:
                loss.backward()
                if K.wgrad_defer:
                    K.wgrad_release()      # (no cut point fired: plain module)
                K.wgrad_flush()            # the last phase (encoder)
        finally:
            self._in_backward = False
            K.wgrad_async = False
            if self.wgrad_async:
                K.join_wgrad_stream()      # weight gradients were produced on the side stream
        self.opt.gather_grads()            # parameters whose gradient came through autograd after all (none on the normal path)
        if self.overlap_comm:
            self._allreduce_chunk(len(sink.chunks) - 1)
            if _capturing() and self._comm_stream is not None:
                torch.cuda.current_stream().wait_stream(self._comm_stream)      # (a capture must end with its forked streams joined)
        return loss.detach(), [p.detach() for p in parts]

    def _weight_tensor(self, term, device):
        """the one-float device tensor the term's kernels read its weight from, made on first use; None with the term off"""
        weight, key = getattr(self, term.name + "_weight"), "_" + term.name
        if weight is not None and getattr(self, key) is None:
            if _capturing():
                raise RuntimeError("the %s weight tensor must exist before the step is captured" % term.name)
            setattr(self, key, torch.full((1,), weight, dtype=torch.float32, device=device))
        return getattr(self, key)

    def set_loss_weight(self, name, w):
        """New weight of the term `name` (cwf.loss_terms) from the next step on, in every step mode: the kernels read it from device
        memory, so a captured step needs no recapture.  Only for a Trainer built with a <name>_weight (the captured step has the term
        or not); the term's other options stay as constructed."""
        term = loss_terms.BY_NAME[name]
        w = loss_terms.check_weight(name, w)
        if w is None or getattr(self, name + "_weight") is None:
            raise ValueError("the %s term is switched on or off at construction (%s_weight=...), not between steps" % (term.title, name))
        setattr(self, name + "_weight", w)              # (remembered for a tensor that does not exist yet)
        if getattr(self, "_" + name) is not None:
            getattr(self, "_" + name).fill_(w)

    def set_boundary_weight(self, w):
        self.set_loss_weight("boundary", w)

    def set_topk_weight(self, w):
        self.set_loss_weight("topk", w)

    def set_focal_weight(self, w):
        self.set_loss_weight("focal", w)

    def set_lovasz_weight(self, w):
        self.set_loss_weight("lovasz", w)

    def _finish_comm(self):
        if not self.comm:
            return
        if self.overlap_comm and (self._graph is None or self._plan is not None):
            for w in self._works:
                w.wait()
            self._works = []
            if self._comm_stream is not None:
                torch.cuda.current_stream().wait_stream(self._comm_stream)
        else:                              # graph replay (collectives are not captured): the whole flat buffer after the replay
            works = [dist.all_reduce(c, async_op=True) for c in self.opt.flat_grad.chunk(4)]
            for w in works:
                w.wait()

    def _capture(self, x, target, edge):
        import ctypes
        import gc
        self._static = (x.clone(), target.clone(), edge.clone())
        for term in loss_terms.TERMS:
            self._weight_tensor(term, x.device)         # (allocated and filled outside the capture)
        want_plan = self.graph_mode == "plan"
        g = torch.cuda.CUDAGraph(keep_graph=True) if want_plan else torch.cuda.CUDAGraph()
        # No cyclic garbage collection inside the capture.  A Trainer and its model form a cycle (model.phase_callback), so an earlier
        # Trainer's plan (streams, events) and kept hipGraph are destroyed by the collector, whenever it runs; when it ran inside this
        # capture, from the autograd thread, the process aborted there.  (torch.cuda.graph itself no longer collects on entry.)
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            # thread-local capture mode: with a process group alive, RCCL's watchdog thread polls events while this thread captures; in
            # the default (global) mode any such call from another thread invalidates the capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._static_out = self._fwd_bwd(*self._static)
        finally:
            if gc_was_on:
                gc.enable()
        self._graph = g
        if want_plan:
            K = kernels_backend()
            plan = ctypes.c_void_p()
            rc = K.lib.cwf_plan_create(ctypes.c_void_p(g.raw_cuda_graph()), ctypes.byref(plan))
            if rc == 0:
                info = (ctypes.c_int * 8)()
                K._call("cwf_plan_info", plan, info)
                self._plan = plan
                self.plan_info = dict(zip(("nodes", "kernels", "markers", "streams", "events", "on_stream0", "on_stream1", "on_streams2plus"), list(info)))
            else:
                # a node kind the launch list cannot express (e.g. a copy node): go on EAGERLY -- the step is GPU-bound, eager launches
                # run it as fast as the plan (they only cost more host time), while hipGraphLaunch of the same capture is 30 % slower
                self.plan_info = {"error": int(rc), "detail": (K.lib.cwf_plan_last_error() or b"").decode(), "fallback": "eager"}
                self._graph = None
                self._static = None
                self.use_graph = False
                self.graph_mode = None

    def _run_plan(self):
        import ctypes
        K = kernels_backend()
        nxt, mk = ctypes.c_int(0), ctypes.c_int(-1)
        main = K._stream()
        cs = self._comm_stream
        cs_raw = cs.cuda_stream if cs is not None else None
        pos = 0
        while True:
            K._call("cwf_plan_run", self._plan, main, cs_raw, pos, ctypes.byref(nxt), ctypes.byref(mk))
            if mk.value < 0:
                break
            lo, hi = self.opt.sink.chunks[mk.value]
            if hi > lo and self.comm and self._last_micro:       # (inside an accumulation window the list just continues)
                with torch.cuda.stream(cs):
                    if self._micro:
                        self.opt.fold(lo, hi)
                    self._works.append(dist.all_reduce(self.opt.flat_grad[lo:hi], async_op=True))
            pos = nxt.value

    def __del__(self):
        try:
            if self._plan is not None:
                kernels_backend().lib.cwf_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    @property
    def static_inputs(self):
        """(x, target, edge) of the captured step, or None before capture: a batch written into these buffers is consumed by the next
        step without a copy."""
        return self._static if self._graph is not None else None

    def step(self, x, target, edge, epoch=0):
        """One optimisation step on a rank-local batch -- with accum_steps = N > 1 one MICRO-step: every N-th call updates the weights
        (learning rate of that call's epoch), the calls before it only accumulate.  Returns this batch's (loss, [five parts]) as
        device tensors (no host sync); a boundary_weight, a topk_weight, a focal_weight and a lovasz_weight each append a part, in that
        order."""
        self._last_micro = self._micro + 1 >= self.accum_steps
        if self._last_micro:
            self.opt.param_groups[0]["lr"] = self.learning_rate(epoch)    # plain float: checkpoints stay weights_only-loadable
        if self.use_graph and self._graph is None and self._eager_steps >= self._graph_warmup:
            torch.cuda.synchronize()
            self._capture(x, target, edge)
        if self._graph is not None and tuple(x.shape) != tuple(self._static[0].shape):
            raise ValueError("this Trainer captured its step for inputs of shape %s; got %s (a captured step is shape-static: use "
                             "use_graph=False for varying shapes)" % (tuple(self._static[0].shape), tuple(x.shape)))
        if self._graph is not None:
            sx, st, se = self._static
            if sx.data_ptr() != x.data_ptr():
                sx.copy_(x)
            if st.data_ptr() != target.data_ptr():
                st.copy_(target)
            if se.data_ptr() != edge.data_ptr():
                se.copy_(edge)
            if self._plan is not None:
                self._run_plan()
            else:
                self._graph.replay()
            loss, parts = self._static_out
        else:
            loss, parts = self._fwd_bwd(x, target, edge)
            self._eager_steps += 1
        if not self._last_micro:
            self.opt.accumulate(first=self._micro == 0)
            self._micro += 1
            self._last_micro = True                     # (direct _fwd_bwd calls outside step() behave as a plain step)
            return loss, parts
        if self._micro and not self._folds_per_chunk():
            self.opt.fold()                             # no collective, or one over the whole buffer after the step: one fold
        self._finish_comm()
        self._micro = 0
        self.opt.advance_host()
        self.opt.launch()
        return loss, parts

    @property
    def updates_done(self):
        """weight updates made so far (not micro-steps); an optimizer state loaded into self.opt restores it"""
        return self.opt._steps

    def learning_rate(self, epoch):
        """The learning rate of the NEXT update if it falls into `epoch`: schedule(init_lr, epoch, end_epoch) times the linear warm-up
        factor min(1, (updates_done + 1) / warmup_steps).  With the defaults this is float(poly_lr(...)), as it always was."""
        lr = schedule_lr(self.schedule, self.init_lr, epoch, self.end_epoch)
        if self.warmup_steps:
            lr *= warmup_factor(self.updates_done, self.warmup_steps)
        return float(lr)

    def _folds_per_chunk(self):
        """the phase slices are all-reduced one by one (each behind its own fold): the condition _finish_comm waits under"""
        return self.comm and self.overlap_comm and (self._graph is None or self._plan is not None)

    def ema_state_dict(self):
        """The model's state_dict() with every parameter replaced by its EMA (buffers copied): what validation and checkpoints
        load in place of the raw weights."""
        if self.opt.ema_decay is None:
            raise RuntimeError("this Trainer keeps no EMA (ema_decay=None)")
        self.opt._ensure()
        ema = {id(p): e for p, e in zip(self.opt._plist, self.opt.ema)}
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for name, p in self.model.named_parameters():
            if id(p) in ema and name in sd:
                sd[name] = ema[id(p)].detach().clone()
        return sd

    def load_ema_state_dict(self, sd):
        """EMA := the parameter entries of `sd` (keys as in the model's state_dict(), with or without the 'module.' prefix)."""
        if self.opt.ema_decay is None:
            raise RuntimeError("this Trainer keeps no EMA (ema_decay=None)")
        self.opt._ensure()
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        ema = {id(p): e for p, e in zip(self.opt._plist, self.opt.ema)}
        with torch.no_grad():
            for name, p in self.model.named_parameters():
                if id(p) in ema:
                    if name not in sd:
                        raise KeyError("EMA state lacks parameter %r" % name)
                    ema[id(p)].copy_(sd[name])

    def validate(self, validator, use_ema=False):
        """validator.run(self.model) (cwf.validation.Validator) between two steps, leaving the training run as it found it.  Every
        model forward calls begin_step, which advances the device dropout counter, in eval mode too, and validate_softmax leaves the
        model in eval mode; so saved before and put back after: `training` of every sub-module, the stem dropout value, and the two
        int64 words of the device generator (device copies, no synchronisation) -- the dropout masks after a validation are those of
        a run that never validated.  The captured step, its static inputs, the optimizer state and the flat gradient are not touched.
        use_ema: the EMA lives in the optimizer and the captured step holds parameter pointers, so the raw parameters are copied
        aside, the EMA is copied INTO the parameter storage (the forward repacks weights from it on every call) and the raw values are
        copied back after the run: parameters and EMA are bit-equal to before.  With more than one rank every rank calls this; it ends
        with the Validator's all_reduce.  Returns the ValidationResult."""
        if self._micro != 0:
            raise ValueError("validate() inside an accumulation window (%d of %d micro-steps done): the window's gradient sum would "
                             "be left waiting; validate after the step that ends the window" % (self._micro, self.accum_steps))
        if use_ema and self.opt.ema_decay is None:
            raise RuntimeError("this Trainer keeps no EMA (ema_decay=None)")
        model = self.model
        modes = [(m, m.training) for m in model.modules()]
        stem = model.Unet_list.InitConv if hasattr(model, "Unet_list") else None
        dropout = None if stem is None else stem.dropout
        rng = kernels_backend().rng(next(model.parameters()).device) if self.cuda else None
        rng_saved = None if rng is None else rng.clone()
        raw = None
        if use_ema:
            self.opt._ensure()
            params = [p.data for p in self.opt._plist]
            raw = [p.clone(memory_format=torch.preserve_format) for p in params]
            torch._foreach_copy_(params, self.opt.ema)
        try:
            return validator.run(model)
        finally:
            if raw is not None:
                torch._foreach_copy_(params, raw)
            self._restore_rng(rng, rng_saved)
            if stem is not None:
                stem.dropout = dropout
            for m, training in modes:
                m.training = training

    @staticmethod
    def _restore_rng(rng, saved):
        if rng is not None:
            rng.copy_(saved)


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def save_checkpoint(path, model, optimizer, epoch, ema=None):
    """train_no_amp.py:248-253: the reference saves the DDP-wrapped model, hence the 'module.' key prefix.  `ema`
    (Trainer.ema_state_dict()) adds a fourth key 'ema_state_dict' with the same prefix; the reference's three stay as they are."""
    sd = {"module." + k: v for k, v in model.state_dict().items()}
    ck = {"epoch": epoch, "state_dict": sd, "optim_dict": optimizer.state_dict()}
    if ema is not None:
        ck["ema_state_dict"] = {"module." + k: v for k, v in ema.items()}
    torch.save(ck, path)


def load_checkpoint(path, model, map_location="cpu", use_ema=False):
    """train_no_amp.py:147-151 (weights only; the reference never restores 'optim_dict' or 'epoch').  use_ema: load the EMA weights
    the checkpoint carries instead of the raw ones."""
    ck = torch.load(path, map_location=map_location, weights_only=True)
    key = "ema_state_dict" if use_ema else "state_dict"
    if use_ema and key not in ck:
        raise KeyError("checkpoint %s carries no 'ema_state_dict' (it was written without --ema_decay): load it with use_ema=False" % path)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in ck[key].items()}
    model.load_state_dict(sd)
    return ck.get("epoch", 0)
