// tests/emu/plan_emu.cpp — the rule of limo-velo_amd/csrc/lv_plan.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The cost bytes by plan_cell_cost, the goals by plan_cell_of, P by plain sweeps of plan_relax over
// the moves plan_move_allowed lets through until nothing changes (forwards and backwards in turn: the fixpoint does not care), the
// paths by plan_walk (which steps with plan_next), counted first and filled second as the kernels do.  tests/test_plan_host.py holds
// its output to tests/plan_ref.py.
//
// stdin, mode 0 (every float as the decimal value of its 32 bits):
//   0
//   origin[3] resolution nx ny nz planar
//   connectivity min_clear_s2
//   n_cost, then the table
//   nx * ny * nz values of s2
//   n_goals, then n x (x y z);  n_starts, then n x (x y z)
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   "field <nx> <ny> <nz>", the cost bytes on one line, P on the next
//   "stats <goals used> <traversable> <reached> <max P>"
//   per start one line: status, cost, the path's length, its cells
// mode 1: n, then n x (pu cu cv w): plan_relax of each, one per line.  mode 2: n, then n values: plan_isqrt of each.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_plan.hpp"

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

int main() {
    const long long mode = read_i();
    if (mode == 1) {
        for (long long n = read_i(); n > 0; --n) {
            const uint32_t pu = (uint32_t)read_i(), cu = (uint32_t)read_i(), cv = (uint32_t)read_i(), w = (uint32_t)read_i();
            printf("%u\n", plan_relax(pu, cu, cv, w));
        }
        return 0;
    }
    if (mode == 2) {
        for (long long n = read_i(); n > 0; --n) printf("%u\n", plan_isqrt((uint32_t)read_i()));
        return 0;
    }
    PlanGrid g{};
    for (int a = 0; a < 3; ++a) g.origin[a] = read_f();
    g.resolution = read_f();
    g.nx = (int)read_i(); g.ny = (int)read_i(); g.nz = (int)read_i();
    g.planar = (int)read_i();
    lv_plan_params pp{};
    pp.connectivity = (int)read_i();
    pp.min_clear_s2 = (int)read_i();
    const size_t n_cost = (size_t)read_i();
    std::vector<uint8_t> table(n_cost);
    for (uint8_t& t : table) t = (uint8_t)read_i();
    const size_t nc = (size_t)g.nx * g.ny * g.nz;
    std::vector<int32_t> s2(nc);
    for (int32_t& s : s2) s = (int32_t)read_i();
    const size_t n_goals = (size_t)read_i();
    std::vector<float> goals(3 * n_goals);
    for (float& x : goals) x = read_f();
    const size_t n_starts = (size_t)read_i();
    std::vector<float> starts(3 * n_starts);
    for (float& x : starts) x = read_f();
    const char* why = plan_check(&pp, table.data(), n_cost, goals.data(), 12, n_goals);
    if (!why) why = plan_check_field(pp.connectivity, g.planar != 0);
    if (why) {
        printf("params bad: %s\n", why);
        return 0;
    }
    printf("params ok\n");
    g.max_m = plan_max_m(pp.connectivity);

    std::vector<uint8_t> cost(nc);   // exactly nc bytes: the sanitizer watches the field's ends
    std::vector<uint32_t> P(nc, PLAN_UNREACHED);
    for (size_t v = 0; v < nc; ++v) cost[v] = (uint8_t)plan_cell_cost(s2[v], pp.min_clear_s2, table.data(), (int)n_cost);
    const PlanView f{cost.data(), P.data(), g.nx, g.ny, g.nz};
    unsigned long long used = 0;
    for (size_t q = 0; q < n_goals; ++q) {
        int i, j, k;
        if (!plan_cell_of(g, &goals[3 * q], i, j, k) || !f.cost(i, j, k)) continue;
        P[f.at(i, j, k)] = 0u;
        ++used;
    }
    bool changed = true;
    for (size_t sweep = 0; changed; ++sweep) {
        if (sweep > nc + 1) { printf("no fixpoint\n"); return 3; }
        changed = false;
        for (size_t n = 0; n < nc; ++n) {
            const size_t v = (sweep & 1) ? nc - 1 - n : n;
            const int i = (int)(v % g.nx), j = (int)((v / g.nx) % g.ny), k = (int)(v / ((size_t)g.nx * g.ny));
            for (int mv = g.planar ? 9 : 0; mv < (g.planar ? 18 : 27); ++mv) {
                int dx, dy, dz;
                const int m = plan_move(mv, dx, dy, dz);
                if (m == 0 || m > g.max_m || !plan_move_allowed(f, i, j, k, dx, dy, dz)) continue;
                const uint32_t cand = plan_relax(f.pot(i + dx, j + dy, k + dz), f.cost(i + dx, j + dy, k + dz), cost[v], plan_weight(m));
                if (plan_edge(f.cost(i + dx, j + dy, k + dz), cost[v], m) != plan_weight(m) * (f.cost(i + dx, j + dy, k + dz) + cost[v])) return 4;
                if (cand < P[v]) {
                    P[v] = cand;
                    changed = true;
                }
            }
        }
    }
    unsigned long long trav = 0, reached = 0, top = 0;
    for (size_t v = 0; v < nc; ++v) {
        trav += cost[v] != 0;
        if (P[v] != PLAN_UNREACHED) {
            ++reached;
            if (P[v] > top) top = P[v];
        }
    }
    printf("field %d %d %d\n", g.nx, g.ny, g.nz);
    for (size_t v = 0; v < nc; ++v) printf("%u ", (unsigned)cost[v]);
    printf("\n");
    for (size_t v = 0; v < nc; ++v) printf("%u ", P[v]);
    printf("\nstats %llu %llu %llu %llu\n", used, trav, reached, top);
    for (size_t q = 0; q < n_starts; ++q) {
        int32_t st = -1, st2 = -1;
        uint32_t pc = 1, pc2 = 1;
        const uint64_t len = plan_walk(g, f, &starts[3 * q], &st, &pc, nullptr);
        std::vector<int32_t> cells(len);   // exactly the counted length
        const uint64_t len2 = plan_walk(g, f, &starts[3 * q], &st2, &pc2, len ? cells.data() : nullptr);
        if (len2 != len || st2 != st || pc2 != pc) { printf("the filling walk differs from the counting one\n"); return 5; }
        printf("%d %u %llu", st, pc, (unsigned long long)len);
        for (int32_t c : cells) printf(" %d", c);
        printf("\n");
    }
    return 0;
}
