// tests/emu/lattice_emu.cpp — the rule of limo-velo_amd/csrc/lv_lattice.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The table by lattice_check, the goals by lat_cell_of, V by plain sweeps in which every state pulls
// lat_relax over the primitives lat_prim_allowed lets through until nothing changes (forwards and backwards in turn: the fixpoint
// does not care), the paths by lat_walk (which steps with lat_next), counted first and filled second as the kernels do.
// tests/test_lattice_host.py holds its output to tests/lattice_ref.py.
//
// stdin, mode 0 (every float as the decimal value of its 32 bits):
//   0
//   origin[3] resolution nx ny
//   H P n_prims, then per record: di dj h_to n_sweep length reserved penalty and the 20 sweep values
//   nx * ny cost bytes
//   n_goals, then n x (x y z h);  n_starts, then n x (x y z h)
// stdout:
//   "params ok" or "params bad: <record, -1 for none>: <why>" (and nothing more)
//   "lattice <nx> <ny> <H> <reach>", V on the next line
//   "stats <goals used> <traversable> <reached> <max V>"
//   per start two lines: status, cost, the path's length, its states; then the primitives taken
// mode 1: n, then n x (pv cu cv length penalty): lat_relax(pv, lat_edge(...)) of each, one per line.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_lattice.hpp"

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

struct Pose {
    float p[3];
    int32_t h;
};

static std::vector<Pose> read_poses() {
    std::vector<Pose> v((size_t)read_i());
    for (Pose& q : v) {
        for (float& x : q.p) x = read_f();
        q.h = (int32_t)read_i();
    }
    return v;
}

int main() {
    const long long mode = read_i();
    if (mode == 1) {
        for (long long n = read_i(); n > 0; --n) {
            const uint32_t pv = (uint32_t)read_i(), cu = (uint32_t)read_i(), cv = (uint32_t)read_i(), len = (uint32_t)read_i(), pen = (uint32_t)read_i();
            printf("%u\n", lat_relax(pv, lat_edge(cu, cv, len, pen)));
        }
        return 0;
    }
    LatGrid g{};
    for (int a = 0; a < 3; ++a) g.origin[a] = read_f();
    g.resolution = read_f();
    g.nx = (int)read_i(); g.ny = (int)read_i(); g.nz = 1;
    lv_lattice_params lp{};
    lp.H = (int)read_i();
    lp.P = (int)read_i();
    const size_t n_prims = (size_t)read_i();
    std::vector<lv_lattice_prim> prims(n_prims);   // exactly n_prims records: the sanitizer watches the table's ends
    for (lv_lattice_prim& r : prims) {
        r.di = (int8_t)read_i(); r.dj = (int8_t)read_i(); r.h_to = (uint8_t)read_i(); r.n_sweep = (uint8_t)read_i();
        r.length = (uint16_t)read_i(); r.reserved = (uint16_t)read_i(); r.penalty = (uint32_t)read_i();
        for (int s = 0; s < LAT_MAX_SWEEP; ++s) { r.sweep[s][0] = (int8_t)read_i(); r.sweep[s][1] = (int8_t)read_i(); }
    }
    const size_t nc = (size_t)g.nx * g.ny;
    std::vector<uint8_t> cost(nc);   // exactly nc bytes
    for (uint8_t& c : cost) c = (uint8_t)read_i();
    const std::vector<Pose> goals = read_poses(), starts = read_poses();
    static_assert(sizeof(Pose) == 16, "a pose record is 16 bytes");
    size_t rec = 0;
    if (const char* why = lattice_check(&lp, prims.data(), n_prims, goals.data(), sizeof(Pose), goals.size(), &rec)) {
        printf("params bad: %lld: %s\n", rec == LAT_NO_RECORD ? -1ll : (long long)rec, why);
        return 0;
    }
    printf("params ok\n");
    g.H = lp.H;
    g.P = lp.P;
    const size_t ns = nc * (size_t)g.H;
    std::vector<uint32_t> V(ns, LAT_UNREACHED);
    const LatView f{cost.data(), V.data(), g.nx, g.ny, 1};
    unsigned long long used = 0;
    for (const Pose& q : goals) {
        int i, j;
        if (q.h < -1 || q.h >= g.H || !lat_cell_of(g, q.p, i, j) || !f.cost(i, j)) continue;
        for (int t = (q.h < 0 ? 0 : q.h); t < (q.h < 0 ? g.H : q.h + 1); ++t) V[lat_at(g, i, j, t)] = 0u;
        ++used;
    }
    bool changed = true;
    for (size_t sweep = 0; changed; ++sweep) {
        if (sweep > ns + 1) { printf("no fixpoint\n"); return 3; }
        changed = false;
        for (size_t n = 0; n < ns; ++n) {
            const size_t s = (sweep & 1) ? ns - 1 - n : n;
            const int i = (int)(s % g.nx), j = (int)((s / g.nx) % g.ny), h = (int)(s / nc);
            for (int p = 0; p < g.P; ++p) {
                const lv_lattice_prim& r = prims[(size_t)h * g.P + p];
                if (!lat_prim_allowed(f, r, i, j)) continue;
                const uint32_t cand = lat_relax(f.pot(i + r.di, j + r.dj, r.h_to), lat_edge(f.cost(i, j), f.cost(i + r.di, j + r.dj), r.length, r.penalty));
                if (cand < V[s]) {
                    V[s] = cand;
                    changed = true;
                }
            }
        }
    }
    unsigned long long trav = 0, reached = 0, top = 0;
    for (size_t s = 0; s < ns; ++s) {
        trav += cost[s % nc] != 0;
        if (V[s] != LAT_UNREACHED) {
            ++reached;
            if (V[s] > top) top = V[s];
        }
    }
    printf("lattice %d %d %d %d\n", g.nx, g.ny, g.H, lat_reach_of(prims.data(), n_prims));
    for (size_t s = 0; s < ns; ++s) printf("%u ", V[s]);
    printf("\nstats %llu %llu %llu %llu\n", used, trav, reached, top);
    for (const Pose& q : starts) {
        int32_t st = -1, st2 = -1;
        uint32_t pc = 1, pc2 = 1;
        const uint64_t len = lat_walk(g, f, prims.data(), q.p, q.h, &st, &pc, nullptr, nullptr);
        std::vector<int32_t> states(len);   // exactly the counted length
        std::vector<uint8_t> taken(len);
        const uint64_t len2 = lat_walk(g, f, prims.data(), q.p, q.h, &st2, &pc2, len ? states.data() : nullptr, len ? taken.data() : nullptr);
        if (len2 != len || st2 != st || pc2 != pc) { printf("the filling walk differs from the counting one\n"); return 5; }
        printf("%d %u %llu", st, pc, (unsigned long long)len);
        for (int32_t s : states) printf(" %d", s);
        printf("\n");
        for (uint8_t t : taken) printf("%u ", (unsigned)t);
        printf("\n");
    }
    return 0;
}
