// tests/emu/frontier_emu.cpp — the rule of limo-velo_amd/csrc/lv_frontier.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The states by fr_state_voxel / fr_state_column, the frontier cells by fr_is_frontier, the
// components by cl_link over the offsets of fr_neighbour (one cell after another: the stand-in's atomics are sequential), the roots
// by cl_root, the numbering by fr_order_key, the records by fr_cluster_record and fr_rep_key, the rank by fr_rank_window.
// tests/test_frontier_host.py holds its output to tests/frontier_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   l_free l_occ nx ny nz                          (the grid)
//   planar k_lo k_hi connectivity min_size
//   nx * ny * nz values of L
//   n_p, then n_p values of P (0, or one per cell of the result);  n_reach, then the reaches
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   "field <nx> <ny> <nz>", the labels on one line
//   "stats <free> <unknown> <frontier> <clusters>"
//   per cluster one line: size first rep centre[3] lo[3] hi[3] sum[3]
//   per reach two lines: best_p of every cluster, best_cell of every cluster
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "lv_frontier.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

static float read_f() {
    unsigned int u = 0;
    if (scanf("%u", &u) != 1) exit(2);
    return __uint_as_float(u);
}
static long long read_i() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) exit(2);
    return v;
}

struct Field {
    const std::vector<uint8_t>& s;   // exactly one byte per cell: the sanitizer watches the field's ends
    int nx, ny, nz;
    int state(int i, int j, int k) const {
        if ((uint32_t)i >= (uint32_t)nx || (uint32_t)j >= (uint32_t)ny || (uint32_t)k >= (uint32_t)nz) return FR_OUTSIDE;
        return s[((size_t)k * ny + j) * nx + i];
    }
};

int main() {
    const float l_free = read_f(), l_occ = read_f();
    const int gx = (int)read_i(), gy = (int)read_i(), gz = (int)read_i();
    lv_frontier_params fp{};
    fp.planar = (int)read_i();
    fp.k_lo = (int)read_i();
    fp.k_hi = (int)read_i();
    fp.connectivity = (int)read_i();
    fp.min_size = (int)read_i();
    std::vector<float> L((size_t)gx * gy * gz);
    for (float& v : L) v = read_f();
    std::vector<uint32_t> P((size_t)read_i());
    for (uint32_t& v : P) v = (uint32_t)read_i();
    std::vector<int> reaches((size_t)read_i());
    for (int& v : reaches) v = (int)read_i();
    if (const char* why = fr_check_params(&fp)) {
        printf("params bad: %s\n", why);
        return 0;
    }
    printf("params ok\n");
    FrontierGrid g{gx, gy, fp.planar ? 1 : gz, fp.planar != 0, plan_max_m(fp.connectivity)};
    const size_t nc = (size_t)g.nx * g.ny * g.nz, plane = (size_t)gx * gy;
    const int k0 = fp.k_lo < 0 ? 0 : fp.k_lo, k1 = fp.k_hi >= gz ? gz - 1 : fp.k_hi;

    std::vector<uint8_t> st(nc);
    for (size_t v = 0; v < nc; ++v)
        st[v] = (uint8_t)(g.planar ? fr_state_column(L.data(), plane, v, k0, k1, l_free, l_occ) : fr_state_voxel(L[v], l_free, l_occ));
    const Field f{st, g.nx, g.ny, g.nz};
    std::vector<uint32_t> parent(nc, CL_NONE);
    unsigned long long n_free = 0, n_unknown = 0, n_frontier = 0;
    for (size_t v = 0; v < nc; ++v) {
        int i, j, k;
        fr_cell_ijk(g, (uint32_t)v, i, j, k);
        n_free += st[v] == FR_FREE;
        n_unknown += st[v] == FR_UNKNOWN;
        if (fr_is_frontier(f, g.planar != 0, i, j, k)) {
            parent[v] = (uint32_t)v;
            ++n_frontier;
        }
    }
    for (size_t v = 0; v < nc; ++v) {
        if (parent[v] == CL_NONE) continue;
        int i, j, k;
        fr_cell_ijk(g, (uint32_t)v, i, j, k);
        for (int mv = 0; mv < 13; ++mv) {
            int dx, dy, dz;
            if (!fr_neighbour(mv, g.max_m, g.planar != 0, dx, dy, dz)) continue;
            if (f.state(i + dx, j + dy, k + dz) == FR_OUTSIDE) continue;
            const size_t u = ((size_t)(k + dz) * g.ny + (j + dy)) * g.nx + (i + dx);
            if (parent[u] != CL_NONE) cl_link(parent.data(), (uint32_t)v, (uint32_t)u);
        }
    }
    // per root: the record's sums
    struct Acc { uint32_t size = 0; uint64_t sum[3] = {0, 0, 0}; int32_t lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {0, 0, 0}; };
    std::vector<uint32_t> root(nc, CL_NONE), dense(nc, CL_NONE), first;
    for (size_t v = 0; v < nc; ++v) {
        if (parent[v] == CL_NONE) continue;
        root[v] = cl_root(parent.data(), (uint32_t)v);
        if (root[v] == v) {
            dense[v] = (uint32_t)first.size();
            first.push_back((uint32_t)v);
        }
    }
    std::vector<Acc> acc(first.size());
    for (size_t v = 0; v < nc; ++v) {
        if (root[v] == CL_NONE) continue;
        Acc& a = acc[dense[root[v]]];   // (a root is the smallest member: numbered before any other member is met)
        int c[3];
        fr_cell_ijk(g, (uint32_t)v, c[0], c[1], c[2]);
        ++a.size;
        for (int x = 0; x < 3; ++x) {
            a.sum[x] += (uint64_t)c[x];
            a.lo[x] = std::min(a.lo[x], c[x]);
            a.hi[x] = std::max(a.hi[x], c[x]);
        }
    }
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    for (size_t d = 0; d < acc.size(); ++d)
        if (acc[d].size >= (uint32_t)fp.min_size) keys.push_back({fr_order_key(acc[d].size, first[d]), (uint32_t)d});
    std::sort(keys.begin(), keys.end());
    const size_t C = keys.size();
    std::vector<int32_t> number(acc.size(), FR_NONE);
    std::vector<lv_frontier_cluster> cl(C);
    std::vector<uint64_t> best(C, ~0ull);
    for (size_t r = 0; r < C; ++r) {
        const uint32_t d = keys[r].second;
        if (cl_key_size(keys[r].first) != acc[d].size || cl_key_root(keys[r].first) != first[d]) return 4;
        number[d] = (int32_t)r;
        fr_cluster_record(cl[r], acc[d].size, first[d], acc[d].sum, acc[d].lo, acc[d].hi);
    }
    std::vector<int32_t> labels(nc, FR_NONE);
    for (size_t v = 0; v < nc; ++v) {
        if (root[v] == CL_NONE) continue;
        const int32_t lab = number[dense[root[v]]];
        labels[v] = lab;
        if (lab < 0) continue;
        int i, j, k;
        fr_cell_ijk(g, (uint32_t)v, i, j, k);
        best[lab] = std::min(best[lab], fr_rep_key(cl[lab].centre, i, j, k, (uint32_t)v));
    }
    for (size_t r = 0; r < C; ++r) cl[r].rep = (int32_t)(uint32_t)best[r];
    printf("field %d %d %d\n", g.nx, g.ny, g.nz);
    for (int32_t v : labels) printf("%d ", v);
    printf("\nstats %llu %llu %llu %zu\n", n_free, n_unknown, n_frontier, C);
    for (const lv_frontier_cluster& c : cl)
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %llu %llu %llu\n", c.size, c.first, c.rep, c.centre[0], c.centre[1], c.centre[2], c.lo[0], c.lo[1],
               c.lo[2], c.hi[0], c.hi[1], c.hi[2], (unsigned long long)c.sum[0], (unsigned long long)c.sum[1], (unsigned long long)c.sum[2]);
    if (P.size() != nc) return 0;
    for (int reach : reaches) {
        std::vector<uint64_t> bid(C, FR_RANK_NONE);
        for (size_t v = 0; v < nc; ++v) {
            if (labels[v] < 0) continue;
            int i, j, k;
            fr_cell_ijk(g, (uint32_t)v, i, j, k);
            bid[labels[v]] = std::min(bid[labels[v]], fr_rank_window(g, P.data(), reach, i, j, k));
        }
        for (uint64_t b : bid) printf("%u ", (uint32_t)(b >> 32));
        printf("\n");
        for (uint64_t b : bid) printf("%d ", (int32_t)(uint32_t)b);
        printf("\n");
    }
    return 0;
}
