// Host-only driver of the launch plan's scheduler (plan_schedule.h) for the address and undefined-behaviour sanitizers:
// `make -C csrc plan_schedule_check` builds it with -fsanitize=address,undefined and runs it.  No HIP, no GPU, no Python.
// It schedules seeded random graphs of 1..40 nodes -- capture-shaped ones (three first-in, first-out chains with fork and join
// edges, markers on the third) and arbitrary DAGs -- plus graphs the scheduler must refuse, and checks the shape of every result;
// what the plan must ORDER is checked by tests/test_plan_schedule_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "plan_schedule.h"

using namespace cwf_plan;

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t m) {                 // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 33) % m;
}

struct Graph {
    std::vector<int> kind, cls, from, to;
};

int pick_kind(bool marker_ok) {
    const uint32_t r = rnd(20);
    if (marker_ok && r < 4) return NK_MARKER;
    if (r < 6) return NK_MEMSET;
    if (r < 8) return NK_EMPTY;
    return NK_KERNEL;
}

Graph capture_shaped(int n) {
    Graph g;
    int last[3] = {-1, -1, -1};
    for (int i = 0; i < n; ++i) {
        const int chain = (int)rnd(8) < 5 ? 0 : (int)rnd(8) < 5 ? 1 : 2;
        const int k = chain == 2 ? (rnd(4) ? NK_MARKER : pick_kind(false)) : pick_kind(false);
        g.kind.push_back(k);
        g.cls.push_back(k != NK_KERNEL ? NC_MAIN : chain == 1 ? (rnd(4) ? NC_SIDE : NC_CONVERSION) : rnd(8) ? NC_MAIN : NC_CONVERSION);
        if (last[chain] >= 0) { g.from.push_back(last[chain]); g.to.push_back(i); }
        for (int c = 0; c < 3; ++c)
            if (c != chain && last[c] >= 0 && rnd(4) == 0) { g.from.push_back(last[c]); g.to.push_back(i); }
        last[chain] = i;
    }
    return g;
}

Graph any_dag(int n) {
    Graph g;
    std::vector<int> label(n);              // creation index of the node at topological rank r: edges need not follow creation order
    for (int i = 0; i < n; ++i) label[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(label[i], label[rnd(i + 1)]);
    g.kind.resize(n);
    g.cls.resize(n);
    for (int i = 0; i < n; ++i) {
        g.kind[i] = pick_kind(true);
        g.cls[i] = g.kind[i] == NK_KERNEL ? (int)rnd(3) : NC_MAIN;
    }
    for (int b = 1; b < n; ++b)
        for (int a = 0; a < b; ++a)
            if (rnd(n) < 2) { g.from.push_back(label[a]); g.to.push_back(label[b]); }
    return g;
}

int fail(const char* what, int graph) {
    fprintf(stderr, "plan_schedule_check: graph %d: %s\n", graph, what);
    return 1;
}

}  // namespace

int main() {
    long waits = 0, nodes = 0;
    for (int t = 0; t < 6000; ++t) {
        const int n = 1 + (int)rnd(40);
        Graph g = t % 2 ? any_dag(n) : capture_shaped(n);
        Schedule S;
        if (!schedule(n, g.kind.data(), g.cls.data(), (int)g.from.size(), g.from.data(), g.to.data(), S)) return fail("refused", t);
        if ((int)S.order.size() != n || (int)S.stream.size() != n || (int)S.wait.size() != n || (int)S.record.size() != n) return fail("sizes", t);
        std::vector<char> seen(n, 0);
        for (int i = 0; i < n; ++i) {
            if (S.order[i] < 0 || S.order[i] >= n || seen[S.order[i]]) return fail("order is no permutation", t);
            seen[S.order[i]] = 1;
            if ((S.stream[i] == -1) != (g.kind[S.order[i]] == NK_MARKER) || S.stream[i] < -1 || S.stream[i] >= MAX_STREAMS) return fail("stream", t);
            if ((int)S.wait[i].size() > MAX_STREAMS) return fail("more waits than source streams", t);
            for (int x : S.wait[i])
                if (x < 0 || x >= i || !S.record[x] || S.stream[x] == S.stream[i]) return fail("wait", t);
            waits += (long)S.wait[i].size();
        }
        for (auto& e : S.edges)
            if (e.first >= e.second) return fail("edge against the order", t);
        nodes += n;
        // the same graph with a back edge (a cycle) and with an edge that names no node
        if (!g.from.empty()) {
            Graph c = g;
            c.from.push_back(g.to[0]);
            c.to.push_back(g.from[0]);
            if (schedule(n, c.kind.data(), c.cls.data(), (int)c.from.size(), c.from.data(), c.to.data(), S)) return fail("cycle accepted", t);
        }
        Graph d = g;
        d.from.push_back(0);
        d.to.push_back(t % 3 ? n : -1);
        if (schedule(n, d.kind.data(), d.cls.data(), (int)d.from.size(), d.from.data(), d.to.data(), S)) return fail("dangling edge accepted", t);
    }
    printf("plan_schedule_check: 6000 graphs, %ld nodes, %ld waits: ok\n", nodes, waits);
    return 0;
}
