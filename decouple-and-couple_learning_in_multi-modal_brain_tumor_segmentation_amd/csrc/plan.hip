// Launch plans: a captured training step re-issued as a plain launch list.
//
// The step (forward + 5 losses + backward + gradient reduces, train_no_amp.py:181-239) is static: fixed patch size, device-side
// token selection, device-resident dropout counters.  cwf.trainer captures it ONCE with stream capture (which records every launch
// of the step -- this library's kernels and the handful of torch fills/copies -- with its arguments and its cross-stream
// dependencies) and hands the resulting hipGraph_t to cwf_plan_create.  The plan orders the graph's nodes topologically (ties in
// the order the host issued them), puts the weight-gradient nodes on a low-priority side stream and everything else on the caller's
// stream, and cwf_plan_run re-issues them: one hipModuleLaunchKernel per kernel node, hipEventRecord / hipStreamWaitEvent for the
// cross-stream edges.  On ROCm 7.2 hipGraphLaunch costs the host ~44 us per
// node of this graph (20.6 ms per step, more than Python's eager enqueue); the plan costs a plain launch per node.
//
// Marker nodes (cwf_plan_marker, captured on the communication stream behind the streams it waits for) cut the list into
// segments: cwf_plan_run stops after a marker, the caller enqueues the data-parallel all-reduce of the finished gradient slice on
// that stream, and continues -- the collective overlaps the rest of backward exactly as in eager mode.
//
// The order, the streams, the waits and the record flags are decided by plan_schedule.h, a host function without a HIP call
// (cwf_plan_schedule exports it for tests on a machine without a GPU); this file maps the hipGraph to its inputs, owns the
// streams and events, issues the list, and lets a test read a built plan back (cwf_plan_describe).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/cwf_hip.h"
#include "plan_schedule.h"

namespace {

__global__ void plan_marker_kernel(int id) { (void)id; }

using namespace cwf_plan;       // NodeKind, NodeClass, MAX_STREAMS, Schedule, schedule(): the pure part, plan_schedule.h
static_assert(NK_KERNEL == CWF_PLAN_KERNEL && NK_MEMSET == CWF_PLAN_MEMSET && NK_EMPTY == CWF_PLAN_EMPTY && NK_MARKER == CWF_PLAN_MARKER, "");
static_assert(NC_MAIN == CWF_PLAN_CLASS_MAIN && NC_SIDE == CWF_PLAN_CLASS_SIDE && NC_CONVERSION == CWF_PLAN_CLASS_CONVERSION, "");

struct PlanNode {
    int kind = NK_EMPTY;
    int stream = 0;             // index into the run's stream set; -1 for markers (the caller's communication stream)
    int marker_id = -1;
    int creation = -1;          // the node's index in the graph's node list (the order the host issued the work in)
    std::string name;           // NK_KERNEL: what hipKernelNameRefByPtr gave (empty if it gave nothing)
    hipKernelNodeParams kp;     // NK_KERNEL (kernelParams / extra point into the graph node: the graph must outlive the plan)
    hipFunction_t fn = nullptr; // resolved once (hipGetFuncBySymbol); nullptr = launch through the host symbol
    hipMemsetParams ms;         // NK_MEMSET
    std::vector<int> wait;      // plan positions (on other streams) this node waits for
    bool record = false;        // a later node on another stream waits for this one
    hipEvent_t ev = nullptr;
};

struct Plan {
    std::vector<PlanNode> nodes;          // in issue order
    std::vector<std::pair<int, int>> edges;   // the graph's edges in plan positions (cwf_plan_describe; the run does not read them)
    std::vector<hipStream_t> owned;       // stream 1, if any (stream 0 is the caller's)
    std::vector<hipEvent_t> join_ev;      // one per owned stream
    hipEvent_t start_ev = nullptr;
    int n_streams = 1, n_kernels = 0, n_markers = 0, n_events = 0;
};

char g_detail[256] = "";       // why the last cwf_plan_create refused a graph (cwf_plan_last_error)

void destroy(Plan* P) {
    for (auto& N : P->nodes)
        if (N.ev) (void)hipEventDestroy(N.ev);
    for (auto e : P->join_ev) (void)hipEventDestroy(e);
    if (P->start_ev) (void)hipEventDestroy(P->start_ev);
    for (auto s : P->owned) (void)hipStreamDestroy(s);
    delete P;
}

}  // namespace

extern "C" int cwf_plan_marker(int id, void* stream) {
    hipLaunchKernelGGL(plan_marker_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, id);
    return (int)hipGetLastError();
}

extern "C" int cwf_plan_create(void* graph_, void** out) {
    if (!graph_ || !out) return CWF_E_BADARG;
    hipGraph_t graph = (hipGraph_t)graph_;
    size_t n = 0, ne = 0;
    hipError_t e = hipGraphGetNodes(graph, nullptr, &n);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return CWF_E_BADARG;
    std::vector<hipGraphNode_t> gn(n);
    e = hipGraphGetNodes(graph, gn.data(), &n);
    if (e != hipSuccess) return (int)e;
    e = hipGraphGetEdges(graph, nullptr, nullptr, &ne);
    if (e != hipSuccess) return (int)e;
    std::vector<hipGraphNode_t> ef(ne), et(ne);
    if (ne) {
        e = hipGraphGetEdges(graph, ef.data(), et.data(), &ne);
        if (e != hipSuccess) return (int)e;
    }
    // node handle -> creation index (the order the host issued the work in)
    std::vector<std::pair<hipGraphNode_t, int>> idx(n);
    for (size_t i = 0; i < n; ++i) idx[i] = {gn[i], (int)i};
    std::sort(idx.begin(), idx.end());
    auto find = [&](hipGraphNode_t h) -> int {
        auto it = std::lower_bound(idx.begin(), idx.end(), std::make_pair(h, -1));
        return (it != idx.end() && it->first == h) ? it->second : -1;
    };
    std::vector<int> efrom(ne), eto(ne);
    for (size_t k = 0; k < ne; ++k) {
        efrom[k] = find(ef[k]);
        eto[k] = find(et[k]);
        if (efrom[k] < 0 || eto[k] < 0) return CWF_E_BADARG;
    }
    // What the scheduler needs of every node, by creation index: its kind and its stream class.  The weight-gradient chain is
    // recognised by its kernels (weight-gradient kernels, their operand conversions and slab reduces).  (A node type the plan cannot
    // express is scheduled as an empty node and refused below, where its position is known.)
    void* marker_fn = (void*)plan_marker_kernel;
    std::vector<hipGraphNodeType> type(n);
    std::vector<hipKernelNodeParams> kparams(n);
    std::vector<const char*> kname(n, nullptr);
    std::vector<int> kind(n, NK_EMPTY), cls(n, NC_MAIN);
    for (size_t i = 0; i < n; ++i) {
        e = hipGraphNodeGetType(gn[i], &type[i]);
        if (e != hipSuccess) return (int)e;
        if (type[i] == hipGraphNodeTypeMemset) kind[i] = NK_MEMSET;
        if (type[i] != hipGraphNodeTypeKernel) continue;
        e = hipGraphKernelNodeGetParams(gn[i], &kparams[i]);
        if (e != hipSuccess) return (int)e;
        if (kparams[i].func == marker_fn && kparams[i].kernelParams) { kind[i] = NK_MARKER; continue; }
        kind[i] = NK_KERNEL;
        const char* nm = kname[i] = hipKernelNameRefByPtr(kparams[i].func, nullptr);
        // (+ the bias-gradient sums of the transposed convs: in_reduce_kernel<0> + stats_channel_sum_kernel, cwf.kernels.channel_sum_to)
        if (nm && (strstr(nm, "wgrad") || strstr(nm, "stats_channel_sum_kernel") ||
                   strstr(nm, "in_reduce_kernelILi0") || strstr(nm, "in_reduce_kernel<0"))) cls[i] = NC_SIDE;
        else if (nm && strstr(nm, "to_bf16_kernel")) cls[i] = NC_CONVERSION;      // decided by the scheduler: a conversion belongs where its readers are
    }
    (void)hipGetLastError();
    Schedule S;
    if (!schedule((int)n, kind.data(), cls.data(), (int)ne, efrom.data(), eto.data(), S)) return CWF_E_BADARG;

    Plan* P = new Plan();
    P->nodes.resize(n);
    P->edges = S.edges;
    bool any_side = false;
    for (size_t i = 0; i < n; ++i) {
        PlanNode& N = P->nodes[i];
        const int c = S.order[i];
        N.creation = c;
        N.stream = S.stream[i];
        N.wait = S.wait[i];
        N.record = S.record[i] != 0;
        any_side = any_side || N.stream == 1;
        const hipGraphNodeType ty = type[c];
        if (ty == hipGraphNodeTypeKernel) {
            N.kp = kparams[c];
            if (kind[c] == NK_MARKER) {
                N.kind = NK_MARKER;
                N.marker_id = *(int*)N.kp.kernelParams[0];
                P->n_markers++;
            } else {
                N.kind = NK_KERNEL;
                if (kname[c]) N.name = kname[c];
                if (hipGetFuncBySymbol(&N.fn, N.kp.func) != hipSuccess) {
                    (void)hipGetLastError();
                    N.fn = nullptr;
                    if (!N.kp.kernelParams) {
                        snprintf(g_detail, sizeof g_detail, "kernel node %zu: no function handle and no parameter array", i);
                        destroy(P);
                        return CWF_E_TOOLARGE;
                    }
                }
                P->n_kernels++;
            }
        } else if (ty == hipGraphNodeTypeMemset) {
            e = hipGraphMemsetNodeGetParams(gn[c], &N.ms);
            if (e != hipSuccess) { destroy(P); return (int)e; }
            if (N.ms.height > 1 || !(N.ms.elementSize == 1 || N.ms.elementSize == 2 || N.ms.elementSize == 4)) {
                snprintf(g_detail, sizeof g_detail, "memset node %zu: elementSize %u width %zu height %zu pitch %zu", i, N.ms.elementSize, N.ms.width, N.ms.height, N.ms.pitch);
                destroy(P);
                return CWF_E_TOOLARGE;
            }
            N.kind = NK_MEMSET;
        } else if (ty == hipGraphNodeTypeMemcpy) {
            // hipMemcpyAsync under capture makes a 1-D copy node, for which the runtime has no parameter getter (the 3-D getter
            // returns garbage on it): refuse copy nodes altogether rather than guess.  The step this library captures has none
            // (its copies are kernels); for a graph that does, the caller drops the capture and goes on with eager steps.
            snprintf(g_detail, sizeof g_detail, "memcpy node at position %zu (copy nodes are not supported: no 1-D parameter getter)", i);
            destroy(P);
            return CWF_E_TOOLARGE;
        } else if (ty == hipGraphNodeTypeEmpty) {
            N.kind = NK_EMPTY;
        } else {
            snprintf(g_detail, sizeof g_detail, "node %zu of type %d (host / child-graph / external-event nodes are not supported)", i, (int)ty);
            destroy(P);
            return CWF_E_TOOLARGE;       // not a step this library captured
        }
    }
    const int n_streams = any_side ? 2 : 1;
    P->n_streams = n_streams;
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    for (int c = 1; c < n_streams; ++c) {
        hipStream_t st;
        hipEvent_t ev;
        // stream 1 = the weight-gradient chain: the runtime's LOW priority (its own hardware-queue pool and the right scheduling hint
        // beside the data-gradient chain, see cwf.kernels.HipBackend.wgrad_stream)
        e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, least);
        if (e != hipSuccess) { destroy(P); return (int)e; }
        P->owned.push_back(st);
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) { destroy(P); return (int)e; }
        P->join_ev.push_back(ev);
    }
    e = hipEventCreateWithFlags(&P->start_ev, hipEventDisableTiming);
    if (e != hipSuccess) { destroy(P); return (int)e; }
    for (auto& N : P->nodes)
        if (N.record) {
            e = hipEventCreateWithFlags(&N.ev, hipEventDisableTiming);
            if (e != hipSuccess) { destroy(P); return (int)e; }
            P->n_events++;
        }
    *out = P;
    return 0;
}

extern "C" const char* cwf_plan_last_error(void) { return g_detail; }

extern "C" int cwf_plan_schedule(int n, const int* kind, const int* cls, int n_edges, const int* edge_from, const int* edge_to,
                                 int* order, int* stream, int* wait_off, int* wait, int* record) {
    if (!order || !stream || !wait_off || !wait || !record) return CWF_E_BADARG;
    Schedule S;
    if (!schedule(n, kind, cls, n_edges, edge_from, edge_to, S)) return CWF_E_BADARG;
    int k = 0;
    for (int i = 0; i < n; ++i) {
        order[i] = S.order[i];
        stream[i] = S.stream[i];
        record[i] = S.record[i];
        wait_off[i] = k;
        for (int x : S.wait[i]) wait[k++] = x;               // (at most one per source stream: k <= MAX_STREAMS * n)
    }
    wait_off[n] = k;
    return 0;
}

extern "C" int cwf_plan_counts(void* plan, int* counts3) {
    if (!plan || !counts3) return CWF_E_BADARG;
    Plan* P = (Plan*)plan;
    size_t waits = 0;
    for (auto& N : P->nodes) waits += N.wait.size();
    counts3[0] = (int)P->nodes.size(); counts3[1] = (int)waits; counts3[2] = (int)P->edges.size();
    return 0;
}

extern "C" int cwf_plan_describe(void* plan, int* kind, int* stream, int* marker_id, int* record, int* creation, int* wait_off,
                                 int* wait, int* edge_from, int* edge_to) {
    if (!plan || (!wait_off) != (!wait) || (!edge_from) != (!edge_to)) return CWF_E_BADARG;
    Plan* P = (Plan*)plan;
    const int n = (int)P->nodes.size();
    int k = 0;
    for (int i = 0; i < n; ++i) {
        const PlanNode& N = P->nodes[i];
        if (kind) kind[i] = N.kind;
        if (stream) stream[i] = N.stream;
        if (marker_id) marker_id[i] = N.marker_id;
        if (record) record[i] = N.record ? 1 : 0;
        if (creation) creation[i] = N.creation;
        if (wait) {
            wait_off[i] = k;
            for (int x : N.wait) wait[k++] = x;
        }
    }
    if (wait) wait_off[n] = k;
    if (edge_from)
        for (size_t j = 0; j < P->edges.size(); ++j) { edge_from[j] = P->edges[j].first; edge_to[j] = P->edges[j].second; }
    return 0;
}

extern "C" int cwf_plan_kernel_name(void* plan, int position, char* buf, int cap) {
    if (!plan || cap < 0 || (cap > 0 && !buf)) return CWF_E_BADARG;
    Plan* P = (Plan*)plan;
    if (position < 0 || position >= (int)P->nodes.size()) return CWF_E_BADARG;
    const std::string& s = P->nodes[position].name;
    if (cap > 0) {
        const size_t m = std::min(s.size(), (size_t)cap - 1);
        memcpy(buf, s.data(), m);
        buf[m] = 0;
    }
    return (int)s.size();
}

extern "C" int cwf_plan_info(void* plan, int* info8) {
    if (!plan || !info8) return CWF_E_BADARG;
    Plan* P = (Plan*)plan;
    int per[MAX_STREAMS] = {0, 0};
    for (auto& N : P->nodes)
        if (N.stream >= 0 && N.stream < MAX_STREAMS) per[N.stream]++;
    info8[0] = (int)P->nodes.size(); info8[1] = P->n_kernels; info8[2] = P->n_markers; info8[3] = P->n_streams;
    info8[4] = P->n_events; info8[5] = per[0]; info8[6] = per[1]; info8[7] = 0;   // (no further streams)
    return 0;
}

// Issues nodes [start, ...) until the list ends or a marker has been processed; sets *next (= the node count when the list is
// finished) and *marker_id (-1 when finished).  main_stream carries chain 0; comm_stream (may be NULL for a plan without markers)
// receives the markers' waits: work the caller enqueues on it after the call is ordered behind everything the marker depended on.
// When the list finishes, main_stream has been made to wait for the side streams.
extern "C" int cwf_plan_run(void* plan, void* main_stream, void* comm_stream, int start, int* next, int* marker_id) {
    if (!plan || !next || !marker_id) return CWF_E_BADARG;
    Plan* P = (Plan*)plan;
    const int n = (int)P->nodes.size();
    if (start < 0 || start > n) return CWF_E_BADARG;
    hipStream_t st[MAX_STREAMS] = {(hipStream_t)main_stream, nullptr};
    for (int c = 1; c < P->n_streams; ++c) st[c] = P->owned[c - 1];
    hipError_t e;
    if (start == 0 && P->n_streams > 1) {
        // the side streams start behind whatever the caller enqueued on the main stream before the step (input copies, optimizer)
        e = hipEventRecord(P->start_ev, st[0]);
        if (e != hipSuccess) return (int)e;
        for (int c = 1; c < P->n_streams; ++c) {
            e = hipStreamWaitEvent(st[c], P->start_ev, 0);
            if (e != hipSuccess) return (int)e;
        }
    }
    for (int i = start; i < n; ++i) {
        PlanNode& N = P->nodes[i];
        if (N.kind == NK_MARKER && !comm_stream) return CWF_E_BADARG;
        hipStream_t s = N.kind == NK_MARKER ? (hipStream_t)comm_stream : st[N.stream];
        for (int w : N.wait) {
            e = hipStreamWaitEvent(s, P->nodes[w].ev, 0);
            if (e != hipSuccess) return (int)e;
        }
        e = hipSuccess;
        switch (N.kind) {
        case NK_KERNEL:
            if (N.fn)
                e = hipModuleLaunchKernel(N.fn, N.kp.gridDim.x, N.kp.gridDim.y, N.kp.gridDim.z, N.kp.blockDim.x, N.kp.blockDim.y,
                                          N.kp.blockDim.z, N.kp.sharedMemBytes, s, N.kp.kernelParams, N.kp.kernelParams ? nullptr : N.kp.extra);
            else
                e = hipLaunchKernel(N.kp.func, N.kp.gridDim, N.kp.blockDim, N.kp.kernelParams, N.kp.sharedMemBytes, s);
            break;
        case NK_MEMSET:
            if (N.ms.elementSize == 1) e = hipMemsetAsync(N.ms.dst, (int)N.ms.value, N.ms.width, s);
            else if (N.ms.elementSize == 2) e = hipMemsetD16Async((hipDeviceptr_t)N.ms.dst, (unsigned short)N.ms.value, N.ms.width, s);
            else e = hipMemsetD32Async((hipDeviceptr_t)N.ms.dst, (int)N.ms.value, N.ms.width, s);
            break;
        default:
            break;
        }
        if (e != hipSuccess) return (int)e;
        if (N.record) {
            e = hipEventRecord(N.ev, s);
            if (e != hipSuccess) return (int)e;
        }
        if (N.kind == NK_MARKER) {
            *next = i + 1;
            *marker_id = N.marker_id;
            return 0;
        }
    }
    for (int c = 1; c < P->n_streams; ++c) {
        e = hipEventRecord(P->join_ev[c - 1], st[c]);
        if (e != hipSuccess) return (int)e;
        e = hipStreamWaitEvent(st[0], P->join_ev[c - 1], 0);
        if (e != hipSuccess) return (int)e;
    }
    *next = n;
    *marker_id = -1;
    return 0;
}

extern "C" int cwf_plan_destroy(void* plan) {
    if (plan) destroy((Plan*)plan);
    return 0;
}
