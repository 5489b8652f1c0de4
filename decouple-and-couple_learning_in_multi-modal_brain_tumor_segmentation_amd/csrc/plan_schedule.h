// The pure part of the launch plan (plan.hip): from a graph's node kinds, stream classes and edges to the issue order, the stream of
// every position, the event waits and the record flags.  No HIP call and no HIP type: cwf_plan_create maps a captured hipGraph to
// these arrays and calls schedule(); cwf_plan_schedule exports it; plan_schedule_check.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace cwf_plan {

enum NodeKind { NK_KERNEL = 0, NK_MEMSET = 1, NK_EMPTY = 3, NK_MARKER = 4 };     // = CWF_PLAN_KERNEL ... CWF_PLAN_MARKER
enum NodeClass { NC_MAIN = 0, NC_SIDE = 1, NC_CONVERSION = 2 };                  // = CWF_PLAN_CLASS_*
const int MAX_STREAMS = 2;      // the caller's stream and the weight-gradient stream

struct Schedule {
    std::vector<int> order;                  // position -> creation index
    std::vector<int> stream;                 // per position: 0, 1, or -1 for a marker (the caller's communication stream)
    std::vector<std::vector<int>> wait;      // per position: the positions (on other streams) it waits for
    std::vector<char> record;                // per position: a later node on another stream waits for this one
    std::vector<std::pair<int, int>> edges;  // the graph's edges in plan positions, in the order given
};

// Nodes are named by creation index (the order the host issued the work in).  cls matters for kernel nodes only and must be 0 on
// every other kind.  false: a kind or class out of range, an edge that names no node, or a cycle; S is then unspecified.
inline bool schedule(int n, const int* kind, const int* cls, int n_edges, const int* edge_from, const int* edge_to, Schedule& S) {
    if (n <= 0 || n_edges < 0 || !kind || !cls || (n_edges && (!edge_from || !edge_to))) return false;
    for (int i = 0; i < n; ++i) {
        if (!(kind[i] == NK_KERNEL || kind[i] == NK_MEMSET || kind[i] == NK_EMPTY || kind[i] == NK_MARKER)) return false;
        if (cls[i] < NC_MAIN || cls[i] > NC_CONVERSION || (cls[i] != NC_MAIN && kind[i] != NK_KERNEL)) return false;
    }
    std::vector<std::vector<int>> succ(n), pred(n);
    for (int k = 0; k < n_edges; ++k) {
        const int a = edge_from[k], b = edge_to[k];
        if (a < 0 || a >= n || b < 0 || b >= n) return false;
        succ[a].push_back(b);
        pred[b].push_back(a);
    }
    // topological order, smallest creation index first
    std::vector<int> indeg(n);
    std::vector<int>& order = S.order;
    order.clear();
    order.reserve(n);
    std::priority_queue<int, std::vector<int>, std::greater<int>> ready;
    for (int i = 0; i < n; ++i) {
        indeg[i] = (int)pred[i].size();
        if (!indeg[i]) ready.push(i);
    }
    while (!ready.empty()) {
        int u = ready.top();
        ready.pop();
        order.push_back(u);
        for (int v : succ[u])
            if (--indeg[v] == 0) ready.push(v);
    }
    if ((int)order.size() != n) return false;
    std::vector<int> pos(n);
    for (int i = 0; i < n; ++i) pos[order[i]] = i;
    S.edges.resize(n_edges);
    for (int k = 0; k < n_edges; ++k) S.edges[k] = {pos[edge_from[k]], pos[edge_to[k]]};

    // The weight-gradient chain (class 1) ALWAYS goes to stream 1, the low-priority stream, wherever the capture had it -- a
    // structural guess that put it on a high-priority stream, or the main chain on the low-priority one, cost 30-40 % of the step
    // (any assignment is correct; the events below carry every cross-stream edge).  A conversion (class 2) belongs where its
    // readers are.
    std::vector<char> side(n);
    for (int i = 0; i < n; ++i) side[i] = (char)cls[i];
    for (int i = n - 1; i >= 0; --i) {                    // (reverse topological order: a conversion feeding a conversion is handled too)
        const int u = order[i];
        if (side[u] != NC_CONVERSION) continue;
        bool all_side = !succ[u].empty();
        for (int v : succ[u]) all_side = all_side && side[v] == NC_SIDE;
        side[u] = all_side ? NC_SIDE : NC_MAIN;
    }
    // Everything that is not part of the weight-gradient chain stays on the caller's stream, in the order the host issued it (a valid
    // topological order: ties above are broken by creation index).  Spreading independent branches over a third stream made every
    // step 60 % SLOWER on this runtime (31 ms per step against 18).
    int waited[MAX_STREAMS + 1][MAX_STREAMS];                 // [waiting stream (MAX_STREAMS = marker stream)][source] -> last position waited for
    for (auto& row : waited) for (int& w : row) w = -1;
    S.stream.assign(n, 0);
    S.wait.assign(n, std::vector<int>());
    S.record.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        const int v = order[i];
        const bool marker = kind[v] == NK_MARKER;
        const int mine = marker ? -1 : side[v] ? 1 : 0;
        S.stream[i] = mine;
        std::vector<int> w;
        for (int p : pred[v]) {
            const int q = pos[p];
            if (kind[p] == NK_MARKER) {                       // a marker orders nothing on the device beyond what IT waited for
                for (int x : S.wait[q])
                    if (S.stream[x] != mine) w.push_back(x);
            } else if (S.stream[q] != mine) {
                w.push_back(q);
            }
        }
        const int me = mine < 0 ? MAX_STREAMS : mine;
        for (int c = 0; c < MAX_STREAMS; ++c) {               // waits are cumulative per source stream: the latest node is enough
            int last = -1;
            for (int x : w)
                if (S.stream[x] == c) last = std::max(last, x);
            if (last > waited[me][c]) {
                S.wait[i].push_back(last);
                if (!marker) waited[me][c] = last;            // (the marker stream is the caller's: assume nothing across calls)
                S.record[last] = 1;
            }
        }
    }
    return true;
}

}  // namespace cwf_plan
