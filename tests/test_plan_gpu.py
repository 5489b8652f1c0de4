"""GPU: cwf_plan_create / cwf_plan_run on small captured graphs made of the library's own kernels.  Each graph is captured the way
Trainer._capture does it (keep_graph, thread-local capture mode, raw_cuda_graph), after every tensor exists and every kernel has run
once eagerly.  Two lines of defence per case: the plan as cwf_plan_describe shows it must pass the happens-before checker of
tests/plan_ref.py and hold the relations the test knows from its own construction (deterministic); and re-issuing it must give the
eager result bit for bit -- all data are small integers in float32 (every sum below 2^24, exact in any order), producers are long
(grad_add over 2^24 floats, the slice read across streams is its tail, written last) and the consumers across a stream are short.
Nothing here replays a graph with hipGraphLaunch: only the plan is under test."""
import ctypes
import gc

import pytest
import torch

import plan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG, SMALL, C = 1 << 24, 1 << 10, 64            # floats of a long producer; of the slice a consumer across streams reads; its channels
BADARG, TOOLARGE = -1, -2


def _ints(n, lo, hi, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(lo, hi + 1, (n,), generator=g, device=DEV).float()


def _tail(t):
    """the last SMALL floats of a long buffer as a channels-last activation [1, 2, 2, 4, C]"""
    return t[-SMALL:].view(1, 2, 2, SMALL // (4 * C), C)


def _capture(step):
    g = torch.cuda.CUDAGraph(keep_graph=True)
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            step()
    finally:
        if gc_was_on:
            gc.enable()
    return g


def _create(hip, g):
    plan = ctypes.c_void_p()
    rc = hip.lib.cwf_plan_create(ctypes.c_void_p(g.raw_cuda_graph()), ctypes.byref(plan))
    return rc, plan


def _describe(hip, plan):
    from cwf import _lib
    desc = _lib.plan_describe(hip.lib, plan)
    info = (ctypes.c_int * 8)()
    hip._call("cwf_plan_info", plan, info)
    assert len(desc["kind"]) == info[0] and desc["kind"].count(R.KERNEL) == info[1] and desc["kind"].count(R.MARKER) == info[2]
    assert sum(desc["record"]) == info[4] and desc["stream"].count(0) == info[5] and desc["stream"].count(1) == info[6]
    assert sorted(desc["creation"]) == list(range(info[0]))
    return desc


def _run(hip, plan, comm=None, after_marker=None):
    """the whole launch list, segment by segment; -> (marker ids in the order they came back, the final `next`)"""
    nxt, mk = ctypes.c_int(0), ctypes.c_int(-1)
    pos, ids = 0, []
    while True:
        hip._call("cwf_plan_run", plan, hip._stream(), comm.cuda_stream if comm is not None else None, pos, ctypes.byref(nxt), ctypes.byref(mk))
        if mk.value < 0:
            return ids, nxt.value
        ids.append(mk.value)
        assert nxt.value > pos
        if after_marker is not None:
            after_marker(mk.value)
        pos = nxt.value


class _SideStream:
    """weight-gradient launches offered with allow_async go to the backend's side stream, as in a Trainer step"""

    def __init__(self, hip):
        self.hip = hip

    def __enter__(self):
        self.hip.wgrad_async = True

    def __exit__(self, *exc):
        self.hip.wgrad_async = False
        self.hip._wg_sync_needed = False


# ------------------------------------------------------------------------------------------------ fork-join
@pytest.fixture(scope="module")
def fork_join(hip):
    """main: t1 = a + b; dy = t1 + b; [side: out = channel sums of dy's tail]; t2 = dy + a; t1 = t2 + b; join; res = out + c"""
    dev = torch.device(DEV)
    a, b = torch.empty(BIG, device=DEV), torch.empty(BIG, device=DEV)
    t1, dy, t2 = (torch.empty(BIG, device=DEV) for _ in range(3))
    out, res, c = torch.empty(C, device=DEV), torch.empty(C, device=DEV), _ints(C, -3, 3, 7)

    def step():
        hip.begin_step(dev)                                  # (zeroes the arena the reduce's double sums come from, as the model's forward does)
        hip.grad_add(a, b, t1)
        hip.grad_add(t1, b, dy)
        hip.channel_sum_to(_tail(dy), out, allow_async=True)
        hip.grad_add(dy, a, t2)
        hip.grad_add(t2, b, t1)
        hip.join_wgrad_stream()
        hip.grad_add(out, c, res)

    inputs = [(_ints(BIG, -2, 2, 11 + i), _ints(BIG, -2, 2, 21 + i)) for i in range(3)]
    eager = []
    with _SideStream(hip):
        for ai, bi in inputs:
            a.copy_(ai)
            b.copy_(bi)
            step()
            torch.cuda.synchronize()
            eager.append([t.clone() for t in (t1, t2, out, res)])
            # (the eager line itself is sane: the sums are those of dy = a + 2 b, their consumer read the finished sums)
            assert torch.equal(out, _tail(ai + 2 * bi).sum(dim=(0, 1, 2, 3))), int((out != _tail(ai + 2 * bi).sum(dim=(0, 1, 2, 3))).sum())
            assert torch.equal(res, out + c), int((res != out + c).sum())
        assert not torch.equal(eager[0][3], eager[1][3])
        g = _capture(step)
    torch.cuda.synchronize()
    # (step is kept for the tensors it holds: the graph's nodes point at dy and c, and a block the allocator has taken back is rewritten
    # by the next tensor that fits into it)
    return dict(graph=g, step=step, a=a, b=b, c=c, outs=(t1, t2, out, res), inputs=inputs, eager=eager)


def _replay_fork_join(hip, fj, plan, n):
    for i in (1, 2, 0):
        fj["a"].copy_(fj["inputs"][i][0])
        fj["b"].copy_(fj["inputs"][i][1])
        for t in fj["outs"]:
            t.fill_(-77.0)
        ids, nxt = _run(hip, plan)
        torch.cuda.synchronize()
        assert ids == [] and nxt == n
        assert torch.equal(fj["outs"][3], fj["outs"][2] + fj["c"]), (i, "res is not out + c", int((fj["outs"][3] != fj["outs"][2] + fj["c"]).sum()))
        for name, got, want in zip(("t1", "t2", "out", "res"), fj["outs"], fj["eager"][i]):
            assert torch.equal(got, want), (i, name, int((got != want).sum()))


def test_fork_join(hip, fork_join):
    """Structure: two streams; in_reduce_kernel<0> and stats_channel_sum_kernel, and only they, on stream 1; the checker passes; the
    producer of dy happens before the reduce and the channel sum before its consumer.  Three replays on new inputs equal eager."""
    rc, plan = _create(hip, fork_join["graph"])
    assert rc == 0 and plan.value, hip.lib.cwf_plan_last_error()
    try:
        desc = _describe(hip, plan)
        pairs = R.check_described(desc)
        side = [desc["name"][i] for i in range(len(desc["name"])) if desc["stream"][i] == 1]
        print("fork-join plan: %d nodes, streams %s, waits %s, %d pairs ordered; stream 1: %s"
              % (len(desc["kind"]), desc["stream"], desc["waits"], pairs, side))
        assert set(desc["stream"]) == {0, 1} and len(side) == 2, side
        reduce_, csum = R.positions(desc, "in_reduce_kernel", 1), R.positions(desc, "stats_channel_sum_kernel", 1)
        adds = R.positions(desc, "grad_add_kernel", 0)
        assert len(reduce_) == 1 and len(csum) == 1 and len(adds) == 5, (reduce_, csum, adds)
        st, w = desc["stream"], desc["waits"]
        assert R.happens_before(st, w, adds[1], reduce_[0])                 # the producer of dy before the reduce that reads it
        assert R.happens_before(st, w, reduce_[0], csum[0])
        assert R.happens_before(st, w, csum[0], adds[4])                    # the channel sum before its consumer
        assert not R.happens_before(st, w, csum[0], adds[2]) and not R.happens_before(st, w, adds[2], reduce_[0])   # ... and the branches stay parallel
        _replay_fork_join(hip, fork_join, plan, len(desc["kind"]))
    finally:
        hip.lib.cwf_plan_destroy(plan)


def test_destroy_then_create_again(hip, fork_join):
    """a plan destroyed (its events, its side stream) and built again from the same graph describes itself alike and still replays"""
    rc, plan = _create(hip, fork_join["graph"])
    assert rc == 0 and plan.value
    first = _describe(hip, plan)
    _run(hip, plan)
    torch.cuda.synchronize()
    assert hip.lib.cwf_plan_destroy(plan) == 0
    rc, plan = _create(hip, fork_join["graph"])
    assert rc == 0 and plan.value
    try:
        assert _describe(hip, plan) == first
        _replay_fork_join(hip, fork_join, plan, len(first["kind"]))
    finally:
        hip.lib.cwf_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ conversions
@pytest.mark.parametrize("reader", ["side only", "main stream too"])
def test_conversion_goes_where_its_readers_are(hip, reader):
    """A 64 -> 64 channel 3x3x3 weight gradient on an 8 x 12 x 16 volume in bf16 mode (wgrad_s1d_kernel on bf16 images, the shape of
    test_dma_weight_gradient_32_channel_groups), handed to the side stream.  'side only': both operand images are made in front of
    the launch, a conversion feeding a conversion feeding the weight gradient -- all on stream 1.  'main stream too': the image of x
    is made on the main stream, which goes on behind it -- that conversion stays on stream 0, the one of dy goes to stream 1."""
    from cwf import functional as CF, kernels, packing as pk
    dev = torch.device(DEV)
    n, size, ch = 1, (8, 12, 16), 64
    nel = n * size[0] * size[1] * size[2] * ch
    p, q, xf, tm = _ints(nel, -1, 1, 31), _ints(nel, -1, 1, 32), torch.empty(nel, device=DEV), torch.full((nel,), -77.0, device=DEV)
    x = xf.view(n, *size, ch)
    dy = _ints(nel, -1, 1, 33).view(n, *size, ch)
    x16 = torch.empty((n, *size, ch), dtype=torch.bfloat16, device=DEV)
    wn = ch * ch * 27
    dw, db, res = (torch.full((k,), -77.0, device=DEV) for k in (wn, ch, wn))           # (filled alike before the eager run and the replay)
    dw0 = _ints(wn, -3, 3, 34)
    spec = CF.ConvSpec(pk.CONV3_S1, ch, ch).to(dev)
    key = ("plan conversions", reader)

    def step():
        hip.grad_add(p, q, xf)                                              # the producer of x
        if reader == "side only":
            hip.wgrad_to(key, pk.CONV3_S1, x, None, None, 1.0, dy, ch, spec.inv_map, dw, db, allow_async=True)
        else:
            hip.to_bf16(x, out=x16)
            hip.wgrad_to(key, pk.CONV3_S1, x, None, None, 1.0, dy, ch, spec.inv_map, dw, db, x16=x16, allow_async=True)
        hip.grad_add(xf, q, tm)                                             # the main stream goes on
        hip.wgrad_flush(dev)
        hip.join_wgrad_stream()
        hip.grad_add(dw, dw0, res)                                          # reads what the side stream made

    kernels.set_precision("bf16x3", wgrad="bf16", dgrad="bf16")
    plan = None
    try:
        assert hip.bf16_operands_ok(pk.CONV3_S1, ch, ch, size[0] * size[1] * size[2]) == 32
        with _SideStream(hip):
            step()
            torch.cuda.synchronize()
            want = [t.clone() for t in (tm, dw, db, res)]
            assert float(dw.abs().max()) > 0 and torch.equal(db, dy.sum(dim=(0, 1, 2, 3)))
            g = _capture(step)
        rc, plan = _create(hip, g)
        assert rc == 0 and plan.value, hip.lib.cwf_plan_last_error()
        desc = _describe(hip, plan)
        R.check_described(desc)
        conv0, conv1 = R.positions(desc, "to_bf16_kernel", 0), R.positions(desc, "to_bf16_kernel", 1)
        wg = R.positions(desc, "wgrad")
        print("%s: conversions on stream 0 %s, on stream 1 %s, weight-gradient kernels %s, waits %s" % (reader, conv0, conv1, wg, desc["waits"]))
        assert len(wg) >= 2 and all(desc["stream"][i] == 1 for i in wg)
        adds = R.positions(desc, "grad_add_kernel", 0)
        assert len(adds) == 3
        st, w = desc["stream"], desc["waits"]
        if reader == "side only":
            assert conv0 == [] and len(conv1) == 2
        else:
            assert len(conv0) == 1 and len(conv1) == 1
            assert R.happens_before(st, w, conv0[0], wg[0])
        assert all(R.happens_before(st, w, adds[0], i) for i in conv0 + conv1) and all(R.happens_before(st, w, i, wg[0]) for i in conv1)
        assert R.happens_before(st, w, wg[-1], adds[2]) and not R.happens_before(st, w, wg[0], adds[1])
        for t in (xf, tm, dw, db, res):
            t.fill_(-77.0)
        x16.fill_(-77.0)
        ids, nxt = _run(hip, plan)
        torch.cuda.synchronize()
        assert ids == [] and nxt == len(desc["kind"])
        for name, got, ref in zip(("tm", "dw", "db", "res"), (tm, dw, db, res), want):
            assert torch.equal(got, ref), (name, int((got != ref).sum()))
    finally:
        if plan is not None and plan.value:
            hip.lib.cwf_plan_destroy(plan)
        kernels.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ markers
def test_markers_cut_the_list_and_order_the_communication_stream(hip):
    """Two cut points, each a marker on a third stream behind the main and the side stream.  The list is run in segments; behind each
    marker a copy of the slice finished there (the tail of g, and the channel sums the side stream made of it) is enqueued on the
    communication stream, standing in for the all-reduce; later segments overwrite both.  The snapshots must hold the eager values
    AT the cut points.  (Before the list goes on, the main stream is made to wait for the copy: protecting the copy's source from
    what follows is the caller's business, as Trainer._finish_comm shows; what the marker must give is everything BEFORE it.)"""
    dev = torch.device(DEV)
    a, b, g_ = _ints(BIG, -2, 2, 41), _ints(BIG, -2, 2, 42), torch.empty(BIG, device=DEV)
    out = torch.empty(C, device=DEV)
    comm = torch.cuda.Stream(device=DEV)

    def cut(k):
        cur = torch.cuda.current_stream()
        comm.wait_stream(cur)
        comm.wait_stream(hip.wgrad_stream(dev))
        with torch.cuda.stream(comm):
            hip._call("cwf_plan_marker", k, hip._stream())
        cur.wait_stream(comm)                                # (what follows overwrites what the side stream is reading)

    def step(at_cut=cut):
        hip.begin_step(dev)
        hip.grad_add(a, b, g_)
        hip.channel_sum_to(_tail(g_), out, allow_async=True)
        at_cut(0)
        hip.grad_add(g_, b, g_)
        hip.channel_sum_to(_tail(g_), out, allow_async=True)
        at_cut(1)
        hip.grad_add(g_, a, g_)
        hip.join_wgrad_stream()

    want = {}

    def eager_cut(k):
        torch.cuda.synchronize()
        want[k] = (g_[-SMALL:].clone(), out.clone())

    plan = None
    try:
        with _SideStream(hip):
            step(eager_cut)
            torch.cuda.synchronize()
            want["end"] = (g_.clone(), out.clone())
            assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[1][0], want["end"][0][-SMALL:])
            assert not torch.equal(want[0][1], want[1][1])
            step()                                           # (the marker kernel and the third stream, once eagerly)
            torch.cuda.synchronize()
            graph = _capture(step)
        rc, plan = _create(hip, graph)
        assert rc == 0 and plan.value, hip.lib.cwf_plan_last_error()
        desc = _describe(hip, plan)
        R.check_described(desc)
        n = len(desc["kind"])
        marks = [i for i in range(n) if desc["kind"][i] == R.MARKER]
        print("marker plan: %d nodes, streams %s, waits %s" % (n, desc["stream"], desc["waits"]))
        assert [desc["marker_id"][i] for i in marks] == [0, 1] and all(desc["stream"][i] == -1 for i in marks)
        assert all(desc["marker_id"][i] == -1 for i in range(n) if i not in marks)
        st, w = desc["stream"], desc["waits"]
        adds, csum = R.positions(desc, "grad_add_kernel", 0), R.positions(desc, "stats_channel_sum_kernel", 1)
        assert len(adds) == 3 and len(csum) == 2
        for k in (0, 1):                                     # the communication stream waits for both streams' work before cut k ...
            assert R.happens_before(st, w, adds[k], marks[k]) and R.happens_before(st, w, csum[k], marks[k])
            assert R.happens_before(st, w, csum[k], adds[k + 1])     # ... and the overwrite behind the marker took its waits over
        snap = {k: (torch.empty(SMALL, device=DEV), torch.empty(C, device=DEV)) for k in (0, 1)}

        def after_marker(k):
            with torch.cuda.stream(comm):
                snap[k][0].copy_(g_[-SMALL:])
                snap[k][1].copy_(out)
            torch.cuda.current_stream().wait_stream(comm)

        for rep in range(2):
            for t in (g_, out, snap[0][0], snap[0][1], snap[1][0], snap[1][1]):
                t.fill_(-77.0)
            ids, nxt = _run(hip, plan, comm, after_marker)
            torch.cuda.synchronize()
            assert ids == [0, 1] and nxt == n
            for k in (0, 1):
                assert torch.equal(snap[k][0], want[k][0]) and torch.equal(snap[k][1], want[k][1]), (rep, k)
            assert torch.equal(g_, want["end"][0]) and torch.equal(out, want["end"][1])
        # argument errors
        nxt, mk = ctypes.c_int(0), ctypes.c_int(0)
        run = lambda cs, start: hip.lib.cwf_plan_run(plan, hip._stream(), cs, start, ctypes.byref(nxt), ctypes.byref(mk))
        assert run(comm.cuda_stream, -1) == BADARG and run(comm.cuda_stream, n + 1) == BADARG
        assert run(comm.cuda_stream, n) == 0 and nxt.value == n and mk.value == -1        # (past the last node: nothing left)
        assert run(None, 0) == BADARG                        # a plan with markers needs the communication stream
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        if plan is not None and plan.value:
            hip.lib.cwf_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ memset nodes, copy nodes
def _hip_runtime():
    rt = ctypes.CDLL("libamdhip64.so")                       # (the runtime the process has loaded already)
    P, S = ctypes.c_void_p, ctypes.c_size_t
    rt.hipMemsetAsync.argtypes = [P, ctypes.c_int, S, P]
    rt.hipMemsetD16Async.argtypes = [P, ctypes.c_ushort, S, P]
    rt.hipMemsetD32Async.argtypes = [P, ctypes.c_int, S, P]
    rt.hipMemcpyAsync.argtypes = [P, P, S, ctypes.c_int, P]
    return rt


def test_memset_nodes_of_every_element_size(hip):
    """hipMemsetAsync / hipMemsetD16Async / hipMemsetD32Async on the capturing stream (odd counts, non-zero values) become memset nodes;
    the plan re-issues them with the right element size, count and value, and a kernel behind one reads what it wrote"""
    rt = _hip_runtime()
    b8 = torch.empty(4099, dtype=torch.uint8, device=DEV)
    b16 = torch.empty(1025, dtype=torch.int16, device=DEV)
    b32, c, res = torch.empty(SMALL + 1, device=DEV), _ints(SMALL + 1, -3, 3, 51), torch.empty(SMALL + 1, device=DEV)

    def step():
        s = ctypes.c_void_p(hip._stream())
        assert rt.hipMemsetAsync(b8.data_ptr(), 0xAB, b8.numel(), s) == 0
        assert rt.hipMemsetD16Async(b16.data_ptr(), 0xBEEF, b16.numel(), s) == 0
        assert rt.hipMemsetD32Async(b32.data_ptr(), 0x40400000, b32.numel(), s) == 0          # 3.0f
        hip.grad_add(b32, c, res)

    def check(what):
        torch.cuda.synchronize()
        assert bool((b8 == 0xAB).all()), what
        assert bool((b16 == 0xBEEF - 0x10000).all()), what
        assert bool((b32 == 3.0).all()) and torch.equal(res, c + 3.0), what

    plan = None
    try:
        step()
        check("eager")
        g = _capture(step)
        rc, plan = _create(hip, g)
        assert rc == 0 and plan.value, hip.lib.cwf_plan_last_error()
        desc = _describe(hip, plan)
        R.check_described(desc)
        print("memset plan: kinds %s streams %s" % (desc["kind"], desc["stream"]))
        assert desc["kind"].count(R.MEMSET) >= 3 and set(desc["stream"]) == {0} and not any(desc["record"])
        ms = [i for i in range(len(desc["kind"])) if desc["kind"][i] == R.MEMSET]
        add = R.positions(desc, "grad_add_kernel")
        assert len(add) == 1 and all(i < add[0] for i in ms) and all(desc["name"][i] == "" for i in ms)
        for rep in range(2):
            b8.fill_(1); b16.fill_(1); b32.fill_(1.0); res.fill_(-77.0)
            ids, nxt = _run(hip, plan)
            assert ids == [] and nxt == len(desc["kind"])
            check("replay %d" % rep)
    finally:
        if plan is not None and plan.value:
            hip.lib.cwf_plan_destroy(plan)


def test_copy_node_is_refused(hip):
    """a device-to-device hipMemcpyAsync under capture is a copy node: cwf_plan_create answers CWF_E_TOOLARGE, names the node, and
    hands no plan back (decided on the host: nothing is launched)"""
    rt = _hip_runtime()
    src, tmp, dst = _ints(SMALL, -3, 3, 61), torch.empty(SMALL, device=DEV), torch.empty(SMALL, device=DEV)

    def step():
        hip.grad_add(src, src, tmp)
        assert rt.hipMemcpyAsync(dst.data_ptr(), tmp.data_ptr(), 4 * SMALL, 3, ctypes.c_void_p(hip._stream())) == 0    # 3 = device to device
        hip.grad_add(dst, src, tmp)

    step()
    torch.cuda.synchronize()
    assert torch.equal(dst, 2 * src) and torch.equal(tmp, 3 * src)
    g = _capture(step)
    rc, plan = _create(hip, g)
    detail = (hip.lib.cwf_plan_last_error() or b"").decode()
    print("refusal: %d, %r" % (rc, detail))
    assert rc == TOOLARGE and plan.value is None
    assert "memcpy node at position 1" in detail, detail
