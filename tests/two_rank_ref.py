"""A simulated data-parallel peer: world size 2 inside ONE process, on one device, with no process group.

Both ranks of a data-parallel run execute the same program, so the second rank can be played by the first: a RECORD pass runs the
step as rank 1 on rank 1's samples and keeps, for every all-reduce, what that rank handed to the collective; a REPLAY pass runs the
step as rank 0 on rank 0's samples and every all-reduce adds what the peer recorded at the same program point.  What the harness sees
of a collective -- which slice of the flat gradient buffer, on which stream, holding which values at the moment the collective
would read them -- is what a one-rank group (an identity collective) cannot show.

Nothing here imports the package: the harness knows torch.distributed's interface and that the Trainer it is attached to has
`opt.flat_grad`; it restates nothing of cwf/trainer.py.

    with SimulatedPeer(rank=1) as rec:                 # record
        tr = Trainer(...); rec.attach(tr); rec.update = 0; tr.step(...)
    with SimulatedPeer(rank=0, peer=rec.contributions()) as rep:      # replay
        ...

`update` labels the program point (the test sets it: "warmup", 0, 1, ...); a slice is keyed by (update, lo, hi).  The fake
all_reduce runs on the stream that is current at the call -- where a real collective is enqueued -- and its work object's wait()
puts the then-current stream behind an event recorded after the peer's contribution was added, as a real work object does.
Every other communication entry point of torch.distributed raises while the harness is active."""
import torch
import torch.distributed as dist

# every entry point of torch.distributed that moves data, waits for peers or manages groups, all_reduce and broadcast aside
UNMODELLED = ("all_gather", "all_gather_coalesced", "all_gather_into_tensor", "all_gather_object", "all_reduce_coalesced", "all_to_all",
              "all_to_all_single", "barrier", "batch_isend_irecv", "broadcast_object_list", "destroy_process_group", "gather",
              "gather_object", "init_process_group", "irecv", "isend", "monitored_barrier", "new_group", "new_subgroups", "recv",
              "recv_object_list", "reduce", "reduce_scatter", "reduce_scatter_tensor", "scatter", "scatter_object_list", "send",
              "send_object_list")


class Unmodelled(AssertionError):
    """a torch.distributed call the harness does not model, or an all_reduce it cannot place"""


class _Work:
    """what all_reduce(async_op=True) returns: wait() orders the caller's current stream behind the finished collective"""

    def __init__(self, event):
        self._event = event
        self.waited = False

    def wait(self, timeout=None):
        if self._event is not None:
            torch.cuda.current_stream().wait_event(self._event)
        self.waited = True
        return True

    def is_completed(self):
        return self._event is None or self._event.query()


class SimulatedPeer:
    def __init__(self, rank, peer=None, world=2):
        """rank: the rank this process plays.  peer: None (record: the collective adds nothing) or the other rank's
        contributions() (replay)."""
        if world != 2 or rank not in (0, 1):
            raise ValueError("the harness plays one of two ranks")
        self.rank, self.world, self.peer = rank, world, peer
        self.update = None              # label of the current program point, set by the test
        self.log = []                   # one dict per all_reduce: update, lo, hi, stream, snapshot, async_op, work
        self.broadcasts = 0
        self._trainer = None
        self._saved = None

    # ------------------------------------------------------------------ the patch
    def __enter__(self):
        names = ("is_initialized", "get_world_size", "get_rank", "broadcast", "all_reduce") + tuple(n for n in UNMODELLED if hasattr(dist, n))
        self._saved = {n: getattr(dist, n) for n in names}
        dist.is_initialized = lambda: True
        dist.get_world_size = lambda group=None: self.world
        dist.get_rank = lambda group=None: self.rank
        dist.broadcast = self._broadcast
        dist.all_reduce = self._all_reduce
        for n in names[5:]:
            setattr(dist, n, self._refuse(n))
        return self

    def __exit__(self, *exc):
        for n, f in self._saved.items():
            setattr(dist, n, f)
        self._saved = None
        return False

    @staticmethod
    def _refuse(name):
        def refuse(*a, **kw):
            raise Unmodelled("torch.distributed.%s reached the simulated-peer harness, which does not model it" % name)
        return refuse

    def attach(self, trainer):
        """the Trainer (built inside the context) whose flat gradient buffer the collectives are located in"""
        self._trainer = trainer
        return trainer

    # ------------------------------------------------------------------ the modelled calls
    def _broadcast(self, tensor, src=0, group=None, async_op=False):
        # both ranks start from the same deterministic weights: nothing to move
        if src != 0 or group is not None or async_op:
            raise Unmodelled("broadcast(src=%r, group=%r, async_op=%r)" % (src, group, async_op))
        self.broadcasts += 1

    def _all_reduce(self, tensor, op=dist.ReduceOp.SUM, group=None, async_op=False):
        if op != dist.ReduceOp.SUM or group is not None:
            raise Unmodelled("all_reduce(op=%r, group=%r): only the default group's SUM is modelled" % (op, group))
        if self._trainer is None:
            raise Unmodelled("all_reduce before a Trainer was attached")
        flat = self._trainer.opt.flat_grad
        if flat is None or tensor.dtype != flat.dtype or tensor.device != flat.device or tensor.dim() != 1 or not tensor.is_contiguous():
            raise Unmodelled("all_reduce of a tensor that is no contiguous slice of the flat gradient buffer")
        byte = tensor.data_ptr() - flat.data_ptr()
        lo = byte // flat.element_size()
        hi = lo + tensor.numel()
        if byte % flat.element_size() or lo < 0 or hi > flat.numel() or tensor.numel() == 0:
            raise Unmodelled("all_reduce of [%d, %d): outside the flat gradient buffer [0, %d)" % (lo, hi, flat.numel()))
        cuda = tensor.is_cuda
        stream = torch.cuda.current_stream(tensor.device) if cuda else None
        snapshot = tensor.clone()                                    # on the current stream: exactly what this rank contributes
        if self.peer is not None:
            key = (self.update, lo, hi)
            if key not in self.peer:
                raise Unmodelled("all_reduce of %r: the peer issued no collective for this slice at this program point (it issued %s)"
                                 % (key, sorted(k[1:] for k in self.peer if k[0] == self.update)))
            other = self.peer[key]
            tensor.add_(other.to(tensor.device) if other.device != tensor.device else other)
        event = None
        if cuda:
            event = torch.cuda.Event()
            event.record(stream)
        work = _Work(event)
        self.log.append(dict(update=self.update, lo=lo, hi=hi, stream=stream, snapshot=snapshot, async_op=bool(async_op), work=work))
        if async_op:
            return work
        work.wait()
        return None

    # ------------------------------------------------------------------ what the test reads
    def calls(self, update):
        """the log entries of one program point, in issue order"""
        return [e for e in self.log if e["update"] == update]

    def contributions(self):
        """{(update, lo, hi): snapshot} for the other rank's replay pass; a slice reduced twice at one program point has no single
        contribution and is refused here"""
        out = {}
        for e in self.log:
            key = (e["update"], e["lo"], e["hi"])
            if key in out:
                raise Unmodelled("slice %r was all-reduced twice at one program point" % (key,))
            out[key] = e["snapshot"]
        return out


def tiling_error(intervals, n):
    """None if the (lo, hi) intervals cover [0, n) exactly once, else a sentence saying what is wrong"""
    at = 0
    for lo, hi in sorted(intervals):
        if lo > at:
            return "gap [%d, %d)" % (at, lo)
        if lo < at:
            return "[%d, %d) overlaps what precedes it (covered up to %d)" % (lo, hi, at)
        if hi <= lo:
            return "empty interval [%d, %d)" % (lo, hi)
        at = hi
    return None if at == n else ("covered up to %d of %d" % (at, n))
