"""The launch plan (csrc/plan.hip, csrc/plan_schedule.h) restated on Python lists, and a happens-before checker for its plans.
Nothing here imports the package.

(a) schedule(): the scheduling rules as the C states them -- the order, the stream of every position, the waits, the record flags.
(b) check_plan(): given a graph (kinds, edges) and ANY plan for it (order, streams, waits, record flags), derive the order in which
    the device must run the nodes from the way cwf_plan_run issues them, and require that every node runs behind every ancestor it
    has in the graph.  It shares no code and no idea with (a): it does not know which waits (a) elides or why, only what the
    device is told.

Nodes are named by creation index (the order the host issued the work in) in the graph and by plan position in a plan."""

KERNEL, MEMSET, EMPTY, MARKER = 0, 1, 3, 4          # CWF_PLAN_*
MAIN, SIDE, CONVERSION = 0, 1, 2                    # CWF_PLAN_CLASS_*
SIDE_NAMES = ("wgrad", "stats_channel_sum_kernel", "in_reduce_kernelILi0", "in_reduce_kernel<0")     # class SIDE, by substring
CONVERSION_NAME = "to_bf16_kernel"                                                                    # class CONVERSION


class BadGraph(ValueError):
    pass


def kernel_class(name):
    """the stream class cwf_plan_create gives a kernel of this name"""
    if any(s in name for s in SIDE_NAMES):
        return SIDE
    return CONVERSION if CONVERSION_NAME in name else MAIN


# ------------------------------------------------------------------------------------------------ (a) the rules
def schedule(kinds, classes, edges):
    """-> (order, stream, waits, record), each indexed by plan position.  BadGraph for a cycle or an edge that names no node."""
    n = len(kinds)
    succ, pred = [[] for _ in range(n)], [[] for _ in range(n)]
    for a, b in edges:
        if not (0 <= a < n and 0 <= b < n):
            raise BadGraph("edge (%d, %d) names no node" % (a, b))
        succ[a].append(b)
        pred[b].append(a)
    # topological order, among the ready nodes always the one issued first
    indeg = [len(p) for p in pred]
    ready = [i for i in range(n) if not indeg[i]]
    order = []
    while ready:
        u = min(ready)
        ready.remove(u)
        order.append(u)
        for v in succ[u]:
            indeg[v] -= 1
            if not indeg[v]:
                ready.append(v)
    if len(order) != n:
        raise BadGraph("cycle")
    pos = {u: i for i, u in enumerate(order)}
    # a conversion goes where ALL its readers are (and it has one); readers are settled first
    side = list(classes)
    for u in reversed(order):
        if side[u] == CONVERSION:
            side[u] = SIDE if succ[u] and all(side[v] == SIDE for v in succ[u]) else MAIN
    stream = [-1 if kinds[u] == MARKER else (1 if side[u] == SIDE else 0) for u in order]
    waits, record = [[] for _ in range(n)], [0] * n
    waited = {}                                           # (waiting stream, source stream) -> last position waited for
    for i, u in enumerate(order):
        want = []
        for p in pred[u]:
            q = pos[p]
            if kinds[p] == MARKER:                        # a marker orders nothing itself: take over what it waited for
                want += [x for x in waits[q] if stream[x] != stream[i]]
            elif stream[q] != stream[i]:
                want.append(q)
        for c in (0, 1):
            from_c = [x for x in want if stream[x] == c]
            if from_c and max(from_c) > waited.get((stream[i], c), -1):
                waits[i].append(max(from_c))
                record[max(from_c)] = 1
                if stream[i] >= 0:                        # (nothing is remembered for the communication stream)
                    waited[(stream[i], c)] = max(from_c)
    return order, stream, waits, record


# ------------------------------------------------------------------------------------------------ (b) the checker
class PlanError(AssertionError):
    """a plan that does not honour its graph; .position = the plan position of the node found wrong (None: the plan as a whole)"""

    def __init__(self, position, message):
        super().__init__("position %s: %s" % (position, message))
        self.position = position


def _ancestors(n, edges):
    """per node the set of its proper ancestors, as bit masks (edges must run forward: a < b)"""
    pred = [[] for _ in range(n)]
    for a, b in edges:
        pred[b].append(a)
    anc = [0] * n
    for b in range(n):
        for a in pred[b]:
            anc[b] |= anc[a] | (1 << a)
    return anc


def check_plan(kinds, edges, order, stream, waits, record, elision=True):
    """kinds [n] and edges [(a, b)] by creation index; order / stream / waits / record by plan position.  Raises PlanError naming the
    first position found wrong; returns the number of (ancestor, node) pairs it verified."""
    n = len(kinds)
    if sorted(order) != list(range(n)) or not (len(stream) == len(waits) == len(record) == n):
        raise PlanError(None, "order is no permutation of the nodes, or the arrays differ in length")
    pos = [0] * n
    for i, u in enumerate(order):
        pos[u] = i
    kind = [kinds[u] for u in order]
    pe = [(pos[a], pos[b]) for a, b in edges]
    # 1. the order: topological, and at every step the ready node with the smallest creation index
    indeg = [0] * n
    succ = [[] for _ in range(n)]
    for a, b in pe:
        indeg[b] += 1
        succ[a].append(b)
    ready = {i for i in range(n) if not indeg[i]}
    for i in range(n):
        if i not in ready:
            raise PlanError(i, "issued before one of its predecessors")
        first = min(ready, key=lambda j: order[j])
        if first != i:
            raise PlanError(i, "node %d issued while node %d, created earlier, was ready" % (order[i], order[first]))
        ready.remove(i)
        for j in succ[i]:
            indeg[j] -= 1
            if not indeg[j]:
                ready.add(j)
    # 2. streams and waits are well formed
    for i in range(n):
        if (stream[i] == -1) != (kind[i] == MARKER) or stream[i] not in (-1, 0, 1):
            raise PlanError(i, "stream %d for kind %d" % (stream[i], kind[i]))
        for x in waits[i]:
            if not (0 <= x < i):
                raise PlanError(i, "waits for position %d, which is not earlier" % x)
            if not record[x]:
                raise PlanError(i, "waits for position %d, which records no event" % x)
    # 3. what the device is told.  cwf_plan_run issues position after position: waits of i on i's stream, then i, then i's event.
    #    Streams run first in, first out (markers share the communication stream), and a wait puts i and everything later on its
    #    stream behind x and everything earlier on x's.  before[i] = every position the device must have finished when i starts.
    before = [0] * n
    last = {}
    for i in range(n):
        m = 0
        if stream[i] in last:
            j = last[stream[i]]
            m |= before[j] | (1 << j)
        for x in waits[i]:
            m |= before[x] | (1 << x)
        before[i] = m
        last[stream[i]] = i
    # 4. every node behind every ancestor that does work or is waited on (a marker launches nothing the device could be behind)
    anc = _ancestors(n, pe)
    pairs = 0
    for i in range(n):
        missing = anc[i] & ~before[i]
        a = 0
        while missing:
            if missing & 1 and kind[a] != MARKER:
                raise PlanError(i, "%s (node %d, stream %d) can start before its ancestor at position %d (node %d, stream %d)"
                                % ("marker" if kind[i] == MARKER else "node", order[i], stream[i], a, order[a], stream[a]))
            missing >>= 1
            a += 1
        pairs += bin(anc[i]).count("1")
    # 5. the stated elision: behind a wait for position x of a source stream, the same stream waits for nothing at or before x
    if elision:
        seen = {}
        for i in range(n):
            if kind[i] == MARKER:
                continue
            if len({stream[x] for x in waits[i]}) != len(waits[i]):
                raise PlanError(i, "two waits for the same source stream: %s" % (waits[i],))
            for x in waits[i]:
                key = (stream[i], stream[x])
                if x <= seen.get(key, -1):
                    raise PlanError(i, "waits for position %d of stream %d though stream %d already waited for position %d"
                                    % (x, stream[x], stream[i], seen[key]))
            for x in waits[i]:
                key = (stream[i], stream[x])
                seen[key] = max(seen.get(key, -1), x)
    return pairs


def happens_before(stream, waits, a, b):
    """does the issue sequence put position b behind position a on the device?  (same derivation as check_plan, for one pair)"""
    before, last = [0] * len(stream), {}
    for i in range(len(stream)):
        m = 0
        if stream[i] in last:
            j = last[stream[i]]
            m |= before[j] | (1 << j)
        for x in waits[i]:
            m |= before[x] | (1 << x)
        before[i] = m
        last[stream[i]] = i
    return bool(before[b] >> a & 1)


def check_described(desc):
    """check_plan on what cwf._lib.plan_describe returned for a built plan (lists by plan position: kind, stream, record, creation,
    waits, name, edges as position pairs), and the stream rule on its kernel names: every kernel on stream 1 has a side-class name or
    is a conversion all of whose successors are on stream 1, and no kernel with a side-class name is on stream 0.  Returns the number
    of (ancestor, node) pairs verified."""
    order = desc["creation"]
    n = len(order)
    kinds = [None] * n
    for i, u in enumerate(order):
        kinds[u] = desc["kind"][i]
    edges = [(order[a], order[b]) for a, b in desc["edges"]]
    pairs = check_plan(kinds, edges, order, desc["stream"], desc["waits"], desc["record"])
    succ = [[] for _ in range(n)]
    for a, b in desc["edges"]:
        succ[a].append(b)
    for i in range(n):
        if desc["kind"][i] != KERNEL:
            if desc["kind"][i] != MARKER and desc["stream"][i] != 0:
                raise PlanError(i, "a node that is no kernel on stream %d" % desc["stream"][i])
            continue
        cls, st = kernel_class(desc["name"][i]), desc["stream"][i]
        if cls == SIDE and st != 1:
            raise PlanError(i, "%s has a side-class name and sits on stream %d" % (desc["name"][i], st))
        if cls == MAIN and st != 0:
            raise PlanError(i, "%s has no side-class name and sits on stream %d" % (desc["name"][i], st))
        if cls == CONVERSION:
            readers_side = bool(succ[i]) and all(desc["stream"][j] == 1 for j in succ[i])
            if (st == 1) != readers_side:
                raise PlanError(i, "conversion on stream %d; its successors are on streams %s" % (st, [desc["stream"][j] for j in succ[i]]))
    return pairs


def positions(desc, substring, stream=None):
    """plan positions of the kernels whose name contains `substring` (on `stream`, if given), in the order the host issued them"""
    hit = [i for i in range(len(desc["name"])) if substring in desc["name"][i] and (stream is None or desc["stream"][i] == stream)]
    return sorted(hit, key=lambda i: desc["creation"][i])


def drop_wait(waits, i, k):
    """a copy of the wait lists without the k-th wait of position i"""
    out = [list(w) for w in waits]
    del out[i][k]
    return out
