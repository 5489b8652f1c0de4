"""CPU: the launch plan's scheduler (cwf_plan_schedule, the host function cwf_plan_create calls) against tests/plan_ref.py -- its
result must equal the Python restatement of the rules exactly, and must pass the happens-before checker, which knows nothing of the
rules.  Hand-written graphs carry every expected stream, wait and record flag in the test; on them and on seeded random graphs a
plan with one wait taken out must fail the checker at that node, or the wait is shown redundant by the checker passing."""
import ctypes
import random

import pytest

import plan_ref as R
from plan_ref import EMPTY, KERNEL, MARKER, MEMSET

K0, K1, K2 = (KERNEL, R.MAIN), (KERNEL, R.SIDE), (KERNEL, R.CONVERSION)
MS, EM, MK = (MEMSET, 0), (EMPTY, 0), (MARKER, 0)
BADARG = -1


def c_schedule(kinds, classes, edges):
    """cwf_plan_schedule -> (rc, order, stream, waits, record)"""
    from cwf import _lib
    lib = _lib.load()
    n, ne = len(kinds), len(edges)
    arr = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    order, stream, record = ((ctypes.c_int * max(n, 1))() for _ in range(3))
    off, wait = (ctypes.c_int * (n + 1))(), (ctypes.c_int * max(2 * n, 1))()
    for a in (order, stream, record, off, wait):
        for i in range(len(a)):
            a[i] = -7                                   # whatever the call leaves untouched is seen
    rc = lib.cwf_plan_schedule(n, arr(kinds), arr(classes), ne, arr([a for a, _ in edges]), arr([b for _, b in edges]),
                               order, stream, off, wait, record)
    if rc:
        return rc, None, None, None, None
    assert off[0] == 0 and all(off[i] <= off[i + 1] for i in range(n)) and off[n] <= 2 * n
    return 0, list(order), list(stream), [list(wait[off[i]:off[i + 1]]) for i in range(n)], list(record)


# name -> (nodes by creation index, edges, order, stream per position, waits per position, record per position,
#          the necessary waits as (position, index in its list))
HAND = {
    # 0 producer, 1 weight gradient beside 2, 3 reads both
    "fork-join": ([K0, K1, K0, K0], [(0, 1), (0, 2), (2, 3), (1, 3)],
                  [0, 1, 2, 3], [0, 1, 0, 0], [[], [0], [], [1]], [1, 1, 0, 0], [(1, 0), (3, 0)]),
    # the side node 2 hangs on marker 1 alone: it takes over the marker's wait for 0
    "side node behind a marker only": ([K0, MK, K1], [(0, 1), (1, 2)],
                                       [0, 1, 2], [0, -1, 1], [[], [0], [0]], [1, 0, 0], [(1, 0), (2, 0)]),
    # marker 3 behind marker 2; 4 on the main stream hangs on marker 3 and must still wait for the side node 1.  Marker 2's wait for 0
    # is implied by its wait for 1 (1 waited for 0), marker 3's by the communication stream's own order: a marker's waits are not elided
    "marker behind a marker": ([K0, K1, MK, MK, K0], [(0, 1), (0, 2), (1, 2), (2, 3), (3, 4)],
                               [0, 1, 2, 3, 4], [0, 1, -1, -1, 0], [[], [0], [0, 1], [0, 1], [1]], [1, 1, 0, 0, 0],
                               [(1, 0), (2, 1), (4, 0)]),
    # the empty node 3 joins the side node 1 and the main node 2; 4 follows it on the same stream
    "empty node as the join": ([K0, K1, K0, EM, K0], [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)],
                               [0, 1, 2, 3, 4], [0, 1, 0, 0, 0], [[], [0], [], [1], []], [1, 1, 0, 0, 0], [(1, 0), (3, 0)]),
    # conversion 1 feeds conversion 2 feeds the weight gradient 3: all three on the side stream; 4 goes on beside them
    "conversion chain to a weight gradient": ([K0, K2, K2, K1, K0], [(0, 1), (1, 2), (2, 3), (0, 4)],
                                              [0, 1, 2, 3, 4], [0, 1, 1, 1, 0], [[], [0], [], [], []], [1, 0, 0, 0, 0], [(1, 0)]),
    # conversion 1 is read by the weight gradient 2 AND by the main-stream kernel 3: it stays on the main stream
    "conversion with a main-stream reader": ([K0, K2, K1, K0], [(0, 1), (1, 2), (1, 3)],
                                             [0, 1, 2, 3], [0, 0, 1, 0], [[], [], [1], []], [0, 1, 0, 0], [(2, 0)]),
    # no side node (a conversion nobody reads stays where it is): one stream, no events
    "no side node": ([K0, MS, EM, K2], [(0, 1), (1, 2), (0, 3)],
                     [0, 1, 2, 3], [0, 0, 0, 0], [[], [], [], []], [0, 0, 0, 0], []),
    "single node": ([K0], [], [0], [0], [[]], [0], []),
    "single side node": ([K1], [], [0], [1], [[]], [0], []),
    # 3 reads 2 (same stream) and 0 (main stream): stream 1 waited for 1 already, which is behind 0 -- no second wait
    "second cross-stream edge elided": ([K0, K0, K1, K1], [(0, 1), (1, 2), (2, 3), (0, 3)],
                                        [0, 1, 2, 3], [0, 0, 1, 1], [[], [], [1], []], [0, 1, 0, 0], [(2, 0)]),
    # an edge against the creation order: 2 before 1; 3 and 4 are ready together and go by creation index
    "creation-index tie-break": ([K0, K1, K0, K0, K0], [(0, 2), (2, 1), (2, 4), (0, 3)],
                                 [0, 2, 1, 3, 4], [0, 0, 1, 0, 0], [[], [], [1], [], []], [0, 1, 0, 0, 0], [(2, 0)]),
    # both directions at once, a memset on the main stream between: 3 (main) reads the side node 1, 4 (side) reads the memset 2
    "waits in both directions": ([K0, K1, MS, K0, K1], [(0, 1), (0, 2), (1, 3), (2, 3), (1, 4), (2, 4)],
                                 [0, 1, 2, 3, 4], [0, 1, 0, 0, 1], [[], [0], [], [1], [2]], [1, 1, 1, 0, 0],
                                 [(1, 0), (3, 0), (4, 0)]),
}


def _split(nodes):
    return [k for k, _ in nodes], [c for _, c in nodes]


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_graph(name):
    """the C result is the plan written out above; the restatement gives the same; the checker accepts it; without any one necessary
    wait the checker fails AT THAT NODE, and without any other single wait it passes (that wait is redundant)"""
    nodes, edges, order, stream, waits, record, necessary = HAND[name]
    kinds, classes = _split(nodes)
    assert c_schedule(kinds, classes, edges) == (0, order, stream, waits, record)
    assert R.schedule(kinds, classes, edges) == (order, stream, waits, record)
    R.check_plan(kinds, edges, order, stream, waits, record)
    every = [(i, k) for i in range(len(waits)) for k in range(len(waits[i]))]
    assert set(necessary) <= set(every)
    for i, k in every:
        less = R.drop_wait(waits, i, k)
        if (i, k) in necessary:
            with pytest.raises(R.PlanError) as err:
                R.check_plan(kinds, edges, order, stream, less, record)
            assert err.value.position == i, (name, i, k, str(err.value))
        else:
            R.check_plan(kinds, edges, order, stream, less, record)


def test_checker_rejects_what_the_plan_states_beyond_ordering():
    """the properties of a plan besides happens-before: a wait for an unrecorded or later position, an order that is topological
    but not creation-index first, a wait the stream's earlier wait implies, a marker with a stream"""
    nodes, edges, order, stream, waits, record, _ = HAND["second cross-stream edge elided"]
    kinds, _ = _split(nodes)
    with pytest.raises(R.PlanError) as err:                       # the elided wait put back
        R.check_plan(kinds, edges, order, stream, [[], [], [1], [0]], [1, 1, 0, 0])
    assert err.value.position == 3 and "already waited" in str(err.value)
    R.check_plan(kinds, edges, order, stream, [[], [], [1], [0]], [1, 1, 0, 0], elision=False)     # (it orders nothing wrongly)
    with pytest.raises(R.PlanError) as err:                       # no event behind position 1
        R.check_plan(kinds, edges, order, stream, waits, [0, 0, 0, 0])
    assert err.value.position == 2 and "records no event" in str(err.value)
    with pytest.raises(R.PlanError) as err:                       # a wait for itself
        R.check_plan(kinds, edges, order, stream, [[], [], [2], []], [0, 1, 1, 0])
    assert err.value.position == 2 and "not earlier" in str(err.value)
    nodes, edges, order, stream, waits, record, _ = HAND["creation-index tie-break"]
    kinds, _ = _split(nodes)
    with pytest.raises(R.PlanError) as err:                       # 4 before 3: topological, but not the order the host issued
        R.check_plan(kinds, edges, [0, 2, 1, 4, 3], stream, waits, record)
    assert err.value.position == 3 and "created earlier" in str(err.value)
    with pytest.raises(R.PlanError) as err:                       # 1 before its predecessor 2
        R.check_plan(kinds, edges, [0, 1, 2, 3, 4], [0, 1, 0, 0, 0], [[], [0], [], [], []], [1, 0, 0, 0, 0])
    assert err.value.position == 1 and "before one of its predecessors" in str(err.value)
    nodes, edges, order, stream, waits, record, _ = HAND["side node behind a marker only"]
    kinds, _ = _split(nodes)
    with pytest.raises(R.PlanError) as err:
        R.check_plan(kinds, edges, order, [0, 0, 1], waits, record)
    assert err.value.position == 1


@pytest.mark.parametrize("nodes,edges", [
    ([K0, K0], [(0, 1), (1, 0)]),                       # a cycle
    ([K0, K0, K0], [(0, 1), (1, 2), (2, 1)]),           # a cycle behind a valid prefix
    ([K0], [(0, 0)]),                                   # a self-edge
    ([K0, K0], [(0, 5)]),                               # an edge that names no node
    ([K0, K0], [(-1, 1)]),
    ([K0, K0], [(0, 2)]),                               # (one past the last)
    ([(2, 0)], []),                                     # no such kind
    ([(KERNEL, 3)], []),                                # no such class
    ([(EMPTY, 1)], []),                                 # a class on a node that is no kernel
    ([], []),                                           # no node
])
def test_refused_graphs(nodes, edges):
    kinds, classes = _split(nodes)
    assert c_schedule(kinds, classes, edges)[0] == BADARG
    if nodes and all(k in (KERNEL, MEMSET, EMPTY, MARKER) and (c == 0 or (k == KERNEL and c in (1, 2))) for k, c in nodes):
        with pytest.raises(R.BadGraph):
            R.schedule(kinds, classes, edges)


# ------------------------------------------------------------------------------------------------ random graphs
def _kind(rng, marker_ok):
    r = rng.random()
    if marker_ok and r < 0.2:
        return MARKER
    return MEMSET if r < 0.3 else EMPTY if r < 0.4 else KERNEL


def capture_shaped(rng):
    """What a stream capture of a training step looks like: three first-in, first-out chains (main, weight gradients, communication)
    with fork and join edges between their current ends; markers on the third; memset and empty nodes; conversions on either of the
    first two."""
    n = rng.randint(1, 40)
    nodes, edges, last = [], [], [None, None, None]
    for i in range(n):
        chain = rng.choices((0, 1, 2), (6, 3, 1))[0]              # (a step has few cut points)
        kind = (MARKER if rng.random() < 0.75 else _kind(rng, False)) if chain == 2 else _kind(rng, False)
        cls = 0
        if kind == KERNEL:
            cls = (R.SIDE if rng.random() < 0.75 else R.CONVERSION) if chain == 1 else (R.CONVERSION if rng.random() < 0.12 else R.MAIN)
        nodes.append((kind, cls))
        if last[chain] is not None:
            edges.append((last[chain], i))
        for c in range(3):
            if c != chain and last[c] is not None and rng.random() < 0.25:
                edges.append((last[c], i))
        last[chain] = i
    return nodes, edges


def any_dag(rng):
    """an arbitrary DAG: kinds and classes at random, edges along a random topological ranking that is NOT the creation order"""
    n = rng.randint(1, 40)
    label = list(range(n))
    rng.shuffle(label)
    nodes = []
    for _ in range(n):
        kind = _kind(rng, True)
        nodes.append((kind, rng.randrange(3) if kind == KERNEL else 0))
    p = rng.choice((0.5, 1.0, 2.0, 4.0)) / n
    edges = [(label[a], label[b]) for b in range(n) for a in range(b) if rng.random() < p]
    rng.shuffle(edges)
    return nodes, edges


N_RANDOM = 2000
FLOOR = 0.8


@pytest.mark.parametrize("gen", [capture_shaped, any_dag], ids=lambda g: g.__name__)
def test_random_graphs_equal_the_restatement_and_pass_the_checker(gen):
    """2000 seeded graphs of 1..40 nodes of each kind: the C result equals the restatement exactly and passes the checker.  Then every
    wait of every plan is taken out, one at a time: the checker either fails at that node or passes, which shows that wait redundant
    (a marker's wait for a position that another of its waits, or the marker before it, already covers: markers' waits are not
    elided).  Share of the deletions the checker flags, measured: capture_shaped 0.907 (8153 of 8989), any_dag 0.832 (7385 of 8878);
    the floor is 0.8.  No non-marker's wait is ever redundant: there the elision is exact."""
    rng = random.Random(20260000 + len(gen.__name__))
    flagged = deletions = n_nodes = 0
    for t in range(N_RANDOM):
        nodes, edges = gen(rng)
        kinds, classes = _split(nodes)
        rc, order, stream, waits, record = c_schedule(kinds, classes, edges)
        assert rc == 0, (t, nodes, edges)
        assert (order, stream, waits, record) == R.schedule(kinds, classes, edges), (t, nodes, edges)
        try:
            R.check_plan(kinds, edges, order, stream, waits, record)
        except R.PlanError as e:
            raise AssertionError("graph %d: %s\nnodes %s\nedges %s" % (t, e, nodes, edges))
        n_nodes += len(nodes)
        for i in range(len(waits)):
            for k in range(len(waits[i])):
                deletions += 1
                try:
                    R.check_plan(kinds, edges, order, stream, R.drop_wait(waits, i, k), record)       # passes: the wait is redundant
                    assert kinds[order[i]] == MARKER, ("a non-marker's redundant wait was not elided", t, i, nodes, edges)
                except R.PlanError as e:
                    assert e.position == i, (t, i, k, str(e), nodes, edges)
                    flagged += 1
    share = flagged / max(deletions, 1)
    print("%s: %d graphs, %d nodes, %d waits, %d of %d single-wait deletions flagged = %.3f"
          % (gen.__name__, N_RANDOM, n_nodes, deletions, flagged, deletions, share))
    assert deletions > N_RANDOM and share >= FLOOR, (flagged, deletions)          # (more than one wait per graph: the set is not idle)
