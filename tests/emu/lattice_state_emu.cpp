// tests/emu/lattice_state_emu.cpp — HOST test of the lattice planner's state rules in VolumeTools (limo-velo_amd/csrc/lv_volumes.hpp:
// the lattice_* methods, the PLAN EDIT row of the stale table, the lattice's shift, and its release in lv_occ_configure / lv_destroy).
// TEST INFRASTRUCTURE ONLY: built by tests/test_lattice_state_host.py into tests/emu/_build/ (once plain, once with
// AddressSanitizer + UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own lv_volumes.hpp and tool headers,
// unchanged, against the stand-in hip_runtime.h next to this file, in the manner of volumes_emu.cpp, with its own stand-ins for the
// stores' member functions that its scenarios reach: each logs its name through the HIP stand-in, returns the code the scenario
// set for it, and on success sets the flags the real one sets and holds one counted allocation.
// Usage: lattice_state_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>

#include "../../limo-velo_amd/csrc/lv_volumes.hpp"

using namespace lv;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define CHECK(...)                                                                                                  \
    do {                                                                                                            \
        if (!(__VA_ARGS__)) {                                                                                       \
            fprintf(stderr, "CHECK FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #__VA_ARGS__, g_err); \
            std::_Exit(1);                                                                                          \
        }                                                                                                           \
    } while (0)

namespace {

std::map<std::string, int> g_rc;   // what a store function returns (absent: LV_OK)
int ran(const char* name, hipStream_t s) {
    emu_hip::call(name, s);
    const auto it = g_rc.find(name);
    return it == g_rc.end() ? LV_OK : it->second;
}

}  // namespace

// ---- the stand-ins (the .hip files' in the product)
void OccStore::release() {
    emu_hip::call("OccStore::release");
    d_L.release();
    *this = OccStore();
}
int OccStore::configure(hipStream_t s, const lv_occupancy_params& p) {
    if (int rc = ran("OccStore::configure", s)) return rc;
    release();
    prm = p;
    grid = occ_grid_of(p);
    for (int a = 0; a < 3; ++a) origin0[a] = p.origin[a];
    n_vox = grid_cells(grid);
    if (int rc = d_L.need(n_vox)) return rc;
    configured = true;
    return LV_OK;
}
int OccStore::clear(hipStream_t s) { return ran("OccStore::clear", s); }
int OccStore::recentre(hipStream_t s, const int32_t*, const int32_t s_new[3], const float origin_new[3], uint64_t out[4]) {
    if (int rc = ran("OccStore::recentre", s)) return rc;
    if (out) out[0] = out[1] = out[2] = out[3] = 0;
    for (int a = 0; a < 3; ++a) {
        shift[a] = s_new[a];
        prm.origin[a] = origin_new[a];
        grid.origin[a] = origin_new[a];
    }
    return LV_OK;
}
void DistStore::release() {
    emu_hip::call("DistStore::release");
    d_s2.release();
    *this = DistStore();
}
int DistStore::build(hipStream_t s, const OccStore& occ, const lv_distance_params& p, const int8_t*, uint64_t*) {
    const int rc = ran("DistStore::build", s);
    built = false;
    if (rc) return rc;
    const DistGrid g = dist_grid_of(occ.grid, p);
    if (int ra = d_s2.need(grid_cells(g))) return ra;
    prm = p;
    grid = g;
    for (int a = 0; a < 3; ++a) origin[a] = occ.grid.origin[a];
    n_vox = grid_cells(g);
    stale = 0;
    built = true;
    return LV_OK;
}
void PlanStore::release() {
    emu_hip::call("PlanStore::release");
    d_pot.release();
    *this = PlanStore();
}
int PlanStore::build(hipStream_t s, const DistStore& dist, const lv_plan_params& p, const uint8_t*, size_t, const void*, size_t, size_t, uint64_t*) {
    const int rc = ran("PlanStore::build", s);
    built = false;
    if (rc) return rc;
    PlanGrid g{};
    g.nx = dist.grid.nx;
    g.ny = dist.grid.ny;
    g.nz = dist.grid.nz;
    g.planar = dist.prm.planar != 0;
    g.max_m = plan_max_m(p.connectivity);
    if (int ra = d_pot.need(dist.n_vox)) return ra;
    prm = p;
    grid = g;
    n_cells = dist.n_vox;
    rounds = 1;
    stale = 0;
    built = true;
    return LV_OK;
}
void FrontierStore::release() { emu_hip::call("FrontierStore::release"); *this = FrontierStore(); }
void RayStore::release() { emu_hip::call("RayStore::release"); *this = RayStore(); }
void RolloutStore::release() { emu_hip::call("RolloutStore::release"); *this = RolloutStore(); }
void MclStore::release() { emu_hip::call("MclStore::release"); *this = MclStore(); }
void TsdfStore::mesh_release() { emu_hip::call("TsdfStore::mesh_release"); mesh = TsdfMesh(); }
void TsdfStore::release() { emu_hip::call("TsdfStore::release"); mesh_release(); *this = TsdfStore(); }
int TsdfStore::recentre(hipStream_t s, const int32_t*, const int32_t*, const float*, uint64_t*) { return ran("TsdfStore::recentre", s); }

// ---- lv_lattice.hip: build() stages, drops `built` "before a buffer goes", and sets its fields last
int LatticeStore::build(hipStream_t s, const PlanStore& plan, const lv_lattice_params& p, const lv_lattice_prim*, const void*, size_t, size_t, uint64_t*) {
    const int rc = ran("LatticeStore::build", s);
    built = false;
    if (rc) return rc;
    LatGrid g{};
    g.nx = plan.grid.nx;
    g.ny = plan.grid.ny;
    g.nz = 1;
    g.H = p.H;
    g.P = p.P;
    const size_t ns = (size_t)g.nx * g.ny * p.H;
    if (int ra = d_V.need(ns)) return ra;
    prm = p;
    grid = g;
    n_cells = (size_t)g.nx * g.ny;
    n_states = ns;
    rounds = 1;
    tile = 16;
    reach = 1;
    stale = 0;
    built = true;
    return LV_OK;
}
int LatticeStore::fetch(hipStream_t s, uint32_t*) { return ran("LatticeStore::fetch", s); }
int LatticeStore::paths(hipStream_t s, const void*, size_t, size_t, int32_t*, uint32_t*, size_t*, int32_t*, uint8_t*, size_t, size_t*) {
    return ran("LatticeStore::paths", s);
}

namespace {

using Calls = std::vector<std::string>;
Calls calls(size_t from, bool frees = false) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i)
        if ((frees && log[i].call == "hipFree") || (log[i].call != "hipMalloc" && log[i].call != "hipFree" && log[i].call != "hipHostMalloc" && log[i].call != "hipHostFree"))
            v.push_back(log[i].call);
    return v;
}
size_t mark() { return emu_hip::state().log.size(); }
long live() { return emu_hip::state().mallocs - emu_hip::state().frees; }

#define REFUSED(call, code, msg)                          \
    do {                                                  \
        g_err[0] = 0;                                     \
        CHECK((call) == (code) && std::string(g_err) == (msg)); \
    } while (0)

const char* const NO_GRID = "no occupancy grid: call lv_occ_configure first";
const char* const NO_PLAN = "no plan: call lv_occ_plan_build first";
const char* const NO_LATTICE = "no lattice: call lv_occ_lattice_build first";
const char* const PLAN_3D = "lv_occ_lattice_build: the plan is 3-D: the lattice runs on a planar plan";

const int NX = 8, NY = 6, NZ = 4;

struct Ctx {
    VolumeTools v;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    uint8_t cost[2] = {1, 1};
    float goal[4] = {0.f, 0.f, 0.f, 0.f};
    lv_lattice_prim prims[4] = {};
    uint64_t st[4] = {7, 7, 7, 7};
    Ctx() {
        prims[0].di = 1;
        prims[0].length = 10;
    }
    ~Ctx() { v.release(); }

    int configure(int nx = NX) {
        lv_occupancy_params p;
        default_occupancy_params(&p);
        p.nx = nx; p.ny = NY; p.nz = NZ;
        return v.occ_configure(s, p);
    }
    int field(bool planar) {
        lv_distance_params p;
        default_distance_params(&p);
        p.planar = planar;
        return v.distance_build(s, p, nullptr);
    }
    int plan(int connectivity) {
        lv_plan_params p;
        default_plan_params(&p);
        p.connectivity = connectivity;
        return v.plan_build(s, p, cost, 2, goal, 12, 1, nullptr);
    }
    int lattice(int H = 2) {
        lv_lattice_params p{H, 2};
        return v.lattice_build(s, p, prims, goal, 16, 1, st);
    }
    int fetch(size_t capacity) {
        uint32_t V[1];
        return v.lattice_fetch(s, V, capacity);
    }
    int paths(size_t stride = 16, bool null_total = false) {
        int32_t status[1];
        uint32_t pc[1];
        size_t off[2], total;
        return v.lattice_paths(s, goal, stride, 1, status, pc, off, nullptr, nullptr, 0, null_total ? nullptr : &total);
    }
    int stale() { return v.lattice.built ? v.lattice.stale : -1; }
};

// what each call asks for, in which order
void order() {
    Ctx c;
    lv_lattice_info info;
    REFUSED(c.lattice(), LV_ESTATE, NO_GRID);
    REFUSED(c.fetch(1 << 20), LV_ESTATE, NO_GRID);
    REFUSED(c.paths(), LV_ESTATE, NO_GRID);
    REFUSED(c.v.lattice_info(&info), LV_ESTATE, NO_GRID);
    REFUSED(c.v.lattice_clear(c.s), LV_ESTATE, NO_GRID);
    CHECK(c.configure() == LV_OK);
    REFUSED(c.lattice(), LV_ESTATE, NO_PLAN);
    REFUSED(c.fetch(1 << 20), LV_ESTATE, NO_LATTICE);
    REFUSED(c.paths(), LV_ESTATE, NO_LATTICE);
    REFUSED(c.v.lattice_info(nullptr), LV_EINVAL, "null argument");
    info.built = info.tile = 9;
    CHECK(c.v.lattice_info(&info) == LV_OK && info.built == 0 && info.nx == 0 && info.H == 0 && info.tile == 0 && info.params.H == 0);
    CHECK(c.field(true) == LV_OK);
    REFUSED(c.lattice(), LV_ESTATE, NO_PLAN);   // (a field is not asked for: the plan is the source)
    CHECK(c.field(false) == LV_OK && c.plan(26) == LV_OK);
    REFUSED(c.lattice(), LV_ESTATE, PLAN_3D);
    CHECK(c.field(true) == LV_OK && c.plan(8) == LV_OK);
    // the state count comes after the states: LV_EINVAL, and the store is not reached
    c.v.plan.grid.nx = 1 << 15;
    c.v.plan.grid.ny = 1 << 10;
    size_t t = mark();
    REFUSED(c.lattice(16), LV_EINVAL, "lv_occ_lattice_build: nx * ny * H = 536870912 states: at most 2^28");
    CHECK(calls(t).empty() && c.st[0] == 7);
    c.v.plan.grid.nx = NX;
    c.v.plan.grid.ny = NY;
    t = mark();
    CHECK(c.lattice() == LV_OK && (calls(t) == Calls{"LatticeStore::build"}));
    CHECK(c.v.lattice_info(&info) == LV_OK);
    CHECK(info.built == 1 && info.nx == NX && info.ny == NY && info.H == 2 && info.P == 2 && info.stale == 0 && info.rounds == 1 && info.tile == 16 &&
          info.reach == 1 && info.params.H == 2 && info.params.P == 2);
    // fetch and paths: the lattice, then their arguments
    REFUSED(c.fetch(NX * NY * 2 - 1), LV_EINVAL, "lv_occ_lattice_fetch: room for 96 values needed");
    t = mark();
    CHECK(c.fetch(NX * NY * 2) == LV_OK && (calls(t) == Calls{"LatticeStore::fetch"}));
    REFUSED(c.paths(12), LV_EINVAL, "lv_occ_lattice_paths: bad start array (stride 12) or null status / cost / offsets / total");
    REFUSED(c.paths(16, true), LV_EINVAL, "lv_occ_lattice_paths: bad start array (stride 16) or null status / cost / offsets / total");
    t = mark();
    CHECK(c.paths() == LV_OK && (calls(t) == Calls{"LatticeStore::paths"}));
    // a plan clear does not take the lattice away: fetch and paths go on answering
    CHECK(c.v.plan_clear(c.s) == LV_OK && c.fetch(96) == LV_OK && c.paths() == LV_OK);
    REFUSED(c.lattice(), LV_ESTATE, NO_PLAN);
    // clear: one synchronise, then the buffers
    t = mark();
    const long before = live();
    CHECK(c.v.lattice_clear(c.s) == LV_OK && (calls(t, true) == Calls{"hipStreamSynchronize", "hipFree"}) && live() == before - 1);
    REFUSED(c.fetch(96), LV_ESTATE, NO_LATTICE);
    CHECK(c.v.lattice_clear(c.s) == LV_OK);   // (nothing to free: fine)
}

// the PLAN EDIT row, the shift stamp, and what does not touch the lattice
void stale() {
    Ctx c;
    CHECK(c.configure() == LV_OK && c.field(true) == LV_OK);
    CHECK(c.plan(8) == LV_OK && c.stale() == -1);   // (a lattice that does not exist is not marked)
    CHECK(c.lattice() == LV_OK && c.stale() == 0);
    // a field edit and a grid edit: the plan says of itself that it is stale
    CHECK(c.field(true) == LV_OK && c.v.plan.stale == 1 && c.stale() == 0);
    CHECK(c.v.occ_clear(c.s) == LV_OK && c.v.dist.stale == 1 && c.stale() == 0);
    CHECK(c.v.distance_clear(c.s) == LV_OK && c.stale() == 0);
    // a plan build refused by its own check is no edit; one that got past it is, whatever the store returns
    CHECK(c.field(true) == LV_OK);
    CHECK(c.plan(26) == LV_EINVAL && c.stale() == 0);
    g_rc["PlanStore::build"] = LV_EHIP;
    CHECK(c.plan(8) == LV_EHIP && !c.v.plan.built && c.stale() == 1);
    g_rc.clear();
    REFUSED(c.lattice(), LV_ESTATE, NO_PLAN);
    CHECK(c.stale() == 1);   // (a refused build leaves the old lattice)
    CHECK(c.plan(8) == LV_OK && c.lattice() == LV_OK && c.stale() == 0);
    CHECK(c.plan(8) == LV_OK && c.stale() == 1);
    CHECK(c.lattice() == LV_OK && c.stale() == 0);
    CHECK(c.v.plan_clear(c.s) == LV_OK && c.stale() == 1);
    // a build that fails in the runtime leaves built = 0 and stamps nothing
    CHECK(c.plan(8) == LV_OK);
    const int32_t d[3] = {2, -1, 0};
    CHECK(c.v.recentre(c.s, LV_VOLUME_OCC, d, nullptr) == LV_OK && c.field(true) == LV_OK && c.plan(8) == LV_OK);
    CHECK(c.v.plan.shift[0] == 2 && c.v.plan.shift[1] == -1 && c.v.lattice.shift[0] == 0 && c.stale() == 1);
    g_rc["LatticeStore::build"] = LV_EHIP;
    CHECK(c.lattice() == LV_EHIP && !c.v.lattice.built && c.v.lattice.shift[0] == 0);
    g_rc.clear();
    lv_lattice_info info;
    CHECK(c.v.lattice_info(&info) == LV_OK && info.built == 0);
    // a successful one stamps the plan's shift; a later recentre of the grid leaves lattice and stamp alone
    CHECK(c.lattice() == LV_OK && c.v.lattice.shift[0] == 2 && c.v.lattice.shift[1] == -1 && c.v.lattice.shift[2] == 0);
    CHECK(c.v.recentre(c.s, LV_VOLUME_OCC, d, nullptr) == LV_OK && c.stale() == 0 && c.v.lattice.shift[0] == 2 && c.v.occ.shift[0] == 4);
    CHECK(c.fetch(96) == LV_OK && c.paths() == LV_OK);
}

// lv_occ_configure releases the lattice after mcl; lv_destroy's release
void configure() {
    Ctx c;
    CHECK(c.configure() == LV_OK && c.field(true) == LV_OK && c.plan(8) == LV_OK && c.lattice() == LV_OK);
    CHECK(live() == 4);   // the grid, the field, the plan, the lattice
    size_t t = mark();
    CHECK(c.configure(NX + 1) == LV_OK);
    // the lattice's release logs nothing of its own: its one buffer is the free between MclStore::release and OccStore::configure
    const Calls got = calls(t, true);
    const Calls want{"hipStreamSynchronize", "DistStore::release", "hipFree", "PlanStore::release", "hipFree", "FrontierStore::release", "RayStore::release",
                     "RolloutStore::release", "MclStore::release", "hipFree", "OccStore::configure", "OccStore::release", "hipFree"};
    CHECK(got == want);
    CHECK(live() == 1 && !c.v.lattice.built && c.v.lattice.d_V.p == nullptr && c.v.lattice.n_states == 0);
    REFUSED(c.fetch(96), LV_ESTATE, NO_LATTICE);
    // a configure that fails in the store has already released it (as it has the field and the plan)
    CHECK(c.field(true) == LV_OK && c.plan(8) == LV_OK && c.lattice() == LV_OK);
    g_rc["OccStore::configure"] = LV_EHIP;
    CHECK(c.configure() == LV_EHIP && !c.v.lattice.built);
    g_rc.clear();
    // release: with a lattice, twice, and of tools that never held anything
    CHECK(c.configure() == LV_OK && c.field(true) == LV_OK && c.plan(8) == LV_OK && c.lattice() == LV_OK && live() == 4);
    c.v.release();
    CHECK(live() == 0 && !c.v.lattice.built);
    c.v.release();
    CHECK(live() == 0);
    VolumeTools v;
    t = mark();
    v.release();
    CHECK(calls(t, true) == (Calls{"RayStore::release", "RolloutStore::release", "MclStore::release", "FrontierStore::release", "PlanStore::release",
                                   "DistStore::release", "OccStore::release", "TsdfStore::release", "TsdfStore::mesh_release"}));
}

// the table check's order before any of this (lattice_check: what lv_occ_lattice_build judges before the context)
void check_order() {
    lv_lattice_params p{2, 2};
    lv_lattice_prim t[4] = {};
    float goal[4] = {0, 0, 0, 0};
    size_t rec = 0;
    t[0].di = 1;
    t[0].length = 10;
    CHECK(lattice_check(&p, t, 4, goal, 16, 1, &rec) == nullptr && rec == LAT_NO_RECORD);
    CHECK(lattice_check(nullptr, t, 4, goal, 16, 1, &rec) != nullptr);
    lv_lattice_params bad{0, 2};
    CHECK(std::string(lattice_check(&bad, nullptr, 0, nullptr, 0, 0, &rec)) == "H: 1..16");   // parameters first
    CHECK(std::string(lattice_check(&p, nullptr, 4, nullptr, 0, 0, &rec)) == "null primitive table");
    CHECK(std::string(lattice_check(&p, t, 3, nullptr, 0, 0, &rec)) == "n_prims: H * P records");
    t[3].reserved = 1;
    CHECK(std::string(lattice_check(&p, t, 4, nullptr, 0, 0, &rec)) == "reserved must be 0" && rec == 3);   // the table before the counts
    t[3].reserved = 0;
    CHECK(std::string(lattice_check(&p, t, 4, nullptr, 16, 0, &rec)) == "n_goals: 1..65536" && rec == LAT_NO_RECORD);
    CHECK(std::string(lattice_check(&p, t, 4, nullptr, 16, 1, &rec)) == "bad goal array (null, or a stride below 16)");
    CHECK(std::string(lattice_check(&p, t, 4, goal, 15, 1, &rec)) == "bad goal array (null, or a stride below 16)");
    default_lattice_params(nullptr);
    default_lattice_params(&p);
    CHECK(p.H == 16 && p.P == 3);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: lattice_state_emu <scenario>\n"); return 2; }
    const std::string s = argv[1];
    if (s == "order") order();
    else if (s == "stale") stale();
    else if (s == "configure") configure();
    else if (s == "check_order") check_order();
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees);
    printf("ok %s\n", s.c_str());
    return 0;
}
