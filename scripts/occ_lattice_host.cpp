// scripts/occ_lattice_host.cpp — the host yardstick of scripts/occ_lattice_timing.py: the lattice planner's rule (lv_lattice.hpp:
// lat_prim_allowed, lat_edge, lat_relax) as a Dijkstra over the reversed graph with a binary heap, on one core.  Built with g++ -O2
// through tests/emu/hip/hip_runtime.h.
//   occ_lattice_host <head> <cost> <prims> <goal states> <V out>
// head: int32 nx, ny, H, P, n_goal_states.  cost: nx * ny bytes.  prims: H * P records of 32 bytes.  goal states: int32 indices.
// Writes V (uint32 per state) and prints the solve's milliseconds (the files' reading and writing are not in it).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <queue>
#include <vector>

#include "lv_lattice.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

template <class T>
static std::vector<T> slurp(const char* path, size_t n) {
    std::vector<T> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %zu items of %s\n", n, path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: occ_lattice_host <head> <cost> <prims> <goal states> <V out>\n"); return 2; }
    const std::vector<int32_t> head = slurp<int32_t>(argv[1], 5);
    const int nx = head[0], ny = head[1], H = head[2], P = head[3];
    const size_t nc = (size_t)nx * ny, ns = nc * H;
    const std::vector<uint8_t> cost = slurp<uint8_t>(argv[2], nc);
    const std::vector<lv_lattice_prim> prims = slurp<lv_lattice_prim>(argv[3], (size_t)H * P);
    const std::vector<int32_t> goals = slurp<int32_t>(argv[4], (size_t)head[4]);
    std::vector<uint32_t> V(ns, LAT_UNREACHED);
    const LatView f{cost.data(), V.data(), nx, ny, 1};
    const auto t0 = std::chrono::steady_clock::now();
    // the records that END in heading h, with the heading they start from
    std::vector<std::vector<std::pair<int, const lv_lattice_prim*>>> into(H);
    for (int h = 0; h < H; ++h)
        for (int p = 0; p < P; ++p)
            if (prims[(size_t)h * P + p].length) into[prims[(size_t)h * P + p].h_to].push_back({h, &prims[(size_t)h * P + p]});
    using Item = std::pair<uint32_t, uint32_t>;   // (V, state)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (int32_t g : goals) {
        V[(size_t)g] = 0u;
        heap.push({0u, (uint32_t)g});
    }
    while (!heap.empty()) {
        const Item top = heap.top();
        heap.pop();
        if (top.first > V[top.second]) continue;
        const int hv = (int)(top.second / nc), jv = (int)((top.second % nc) / nx), iv = (int)(top.second % nx);
        const uint32_t cv = cost[top.second % nc];
        for (const auto& e : into[hv]) {
            const lv_lattice_prim& r = *e.second;
            const int iu = iv - r.di, ju = jv - r.dj;
            if (!lat_prim_allowed(f, r, iu, ju)) continue;
            const size_t u = lat_at(f, iu, ju, e.first);
            const uint32_t cand = lat_relax(top.first, lat_edge(f.cost(iu, ju), cv, r.length, r.penalty));
            if (cand < V[u]) {
                V[u] = cand;
                heap.push({cand, (uint32_t)u});
            }
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE* out = fopen(argv[5], "wb");
    if (!out || fwrite(V.data(), sizeof(uint32_t), ns, out) != ns) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
    fclose(out);
    printf("%.3f\n", ms);
    return 0;
}
