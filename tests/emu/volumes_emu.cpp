// tests/emu/volumes_emu.cpp — HOST test of VolumeTools (limo-velo_amd/csrc/lv_volumes.hpp): what each volume call asks for, what
// it marks stale and when, which shift each product remembers, and what is freed in which order.
// TEST INFRASTRUCTURE ONLY: built by tests/test_volumes_host.py into tests/emu/_build/ (once plain, once with AddressSanitizer +
// UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own lv_volumes.hpp and tool headers, unchanged, against
// the stand-in hip_runtime.h next to this file.  The stores' member functions (the .hip files' in the product) are stand-ins
// here: each logs its name through the HIP stand-in, returns the code the scenario set for it, and on success sets exactly the
// flags the real one sets and holds one counted allocation, so a scenario asserts the order of what ran and what is left.
// Usage: volumes_emu <scenario>; exit 0 = pass.
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

// (variadic: a braced list of calls inside the condition carries commas)
#define CHECK(...)                                                                                                  \
    do {                                                                                                            \
        if (!(__VA_ARGS__)) {                                                                                       \
            fprintf(stderr, "CHECK FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #__VA_ARGS__, g_err); \
            std::_Exit(1);                                                                                          \
        }                                                                                                           \
    } while (0)

namespace {

std::map<std::string, int> g_rc;   // what a store function returns (absent: LV_OK)
uint64_t g_marked = 0;             // OccStore::mark's out[2]: the voxels it wrote
int ran(const char* name, hipStream_t s) {
    emu_hip::call(name, s);
    const auto it = g_rc.find(name);
    return it == g_rc.end() ? LV_OK : it->second;
}

}  // namespace

// ---- the stand-ins of lv_occupancy.hip
void OccStore::release() {   // OccStore::release: every buffer, then *this = OccStore()
    emu_hip::call("OccStore::release");
    d_L.release();
    *this = OccStore();
}
int OccStore::configure(hipStream_t s, const lv_occupancy_params& p) {   // OccStore::configure: release(), the shape, configured = true last
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
int OccStore::integrate(hipStream_t s, const lv_view*, size_t, uint64_t*) { return ran("OccStore::integrate", s); }
int OccStore::query(hipStream_t s, const void*, size_t, size_t, float*) { return ran("OccStore::query", s); }
int OccStore::project(hipStream_t s, int, int, int8_t*) { return ran("OccStore::project", s); }
int OccStore::fetch(hipStream_t s, float*) { return ran("OccStore::fetch", s); }
int OccStore::load(hipStream_t s, const float*) { return ran("OccStore::load", s); }
int OccStore::recentre(hipStream_t s, const int32_t*, const int32_t s_new[3], const float origin_new[3], uint64_t out[4]) {
    if (int rc = ran("OccStore::recentre", s)) return rc;
    if (out) { out[0] = n_vox - 1; out[1] = 1; out[2] = 1; out[3] = 0; }
    for (int a = 0; a < 3; ++a) {   // OccStore::recentre's last loop
        shift[a] = s_new[a];
        prm.origin[a] = origin_new[a];
        grid.origin[a] = origin_new[a];
    }
    return LV_OK;
}
int OccStore::mark(hipStream_t s, const lv_occ_mark_params&, const int*, const int*, const void*, uint32_t, const void*, size_t, size_t, uint64_t out[4]) {
    if (int rc = ran("OccStore::mark", s)) return rc;
    out[0] = 11; out[1] = 7; out[2] = g_marked; out[3] = 2;
    return LV_OK;
}

// ---- lv_distance.hip
void DistStore::release() {   // DistStore::release
    emu_hip::call("DistStore::release");
    d_s2.release();
    *this = DistStore();
}
int DistStore::build(hipStream_t s, const OccStore& occ, const lv_distance_params& p, const int8_t*, uint64_t*) {
    const int rc = ran("DistStore::build", s);
    built = false;   // DistStore::build: "before a buffer goes, and until the passes are through"
    if (rc) return rc;
    const DistGrid g = dist_grid_of(occ.grid, p);
    if (int ra = d_s2.need(grid_cells(g))) return ra;
    prm = p;   // ... and its last lines
    grid = g;
    for (int a = 0; a < 3; ++a) origin[a] = occ.grid.origin[a];
    n_vox = grid_cells(g);
    stale = 0;
    built = true;
    return LV_OK;
}
int DistStore::fetch(hipStream_t s, int32_t*, float*) { return ran("DistStore::fetch", s); }
int DistStore::query(hipStream_t s, const void*, size_t, size_t, float*, float*) { return ran("DistStore::query", s); }

// ---- lv_plan.hip
void PlanStore::release() {   // PlanStore::release
    emu_hip::call("PlanStore::release");
    d_pot.release();
    *this = PlanStore();
}
int PlanStore::build(hipStream_t s, const DistStore& dist, const lv_plan_params& p, const uint8_t*, size_t, const void*, size_t, size_t, uint64_t*) {
    const int rc = ran("PlanStore::build", s);
    built = false;   // PlanStore::build: "before a buffer goes"
    if (rc) return rc;
    PlanGrid g{};   // ... its first lines
    g.nx = dist.grid.nx;
    g.ny = dist.grid.ny;
    g.nz = dist.grid.nz;
    g.planar = dist.prm.planar != 0;
    g.max_m = plan_max_m(p.connectivity);
    if (int ra = d_pot.need(dist.n_vox)) return ra;
    prm = p;   // ... and its last
    grid = g;
    n_cells = dist.n_vox;
    rounds = 1;
    stale = 0;
    built = true;
    return LV_OK;
}
int PlanStore::fetch(hipStream_t s, uint32_t*, uint8_t*) { return ran("PlanStore::fetch", s); }
int PlanStore::paths(hipStream_t s, const void*, size_t, size_t, int32_t*, uint32_t*, size_t*, int32_t*, size_t, size_t*) { return ran("PlanStore::paths", s); }

// ---- lv_frontier.hip
void FrontierStore::release() {   // FrontierStore::release
    emu_hip::call("FrontierStore::release");
    d_labels.release();
    *this = FrontierStore();
}
int FrontierStore::build(hipStream_t s, const OccStore& occ, const lv_frontier_params& p, uint64_t*) {
    const int rc = ran("FrontierStore::build", s);
    built = false;   // FrontierStore::build: "before a buffer goes"
    n_clusters = 0;
    if (rc) return rc;
    FrontierGrid g{};   // ... its first lines
    g.nx = occ.grid.nx;
    g.ny = occ.grid.ny;
    g.nz = p.planar ? 1 : occ.grid.nz;
    g.planar = p.planar != 0;
    g.max_m = plan_max_m(p.connectivity);
    if (int ra = d_labels.need(grid_cells(g))) return ra;
    prm = p;   // ... and its last
    grid = g;
    n_cells = grid_cells(g);
    n_clusters = 3;
    stale = 0;
    built = true;
    return LV_OK;
}
int FrontierStore::fetch(hipStream_t s, int32_t*) { return ran("FrontierStore::fetch", s); }
int FrontierStore::clusters(hipStream_t s, lv_frontier_cluster*) { return ran("FrontierStore::clusters", s); }
int FrontierStore::rank(hipStream_t s, const PlanStore&, int, uint32_t*, int32_t*) { return ran("FrontierStore::rank", s); }

// ---- lv_ray.hip (both calls go through RayStore::classify, which packs the states once: packed = true)
void RayStore::release() {   // RayStore::release
    emu_hip::call("RayStore::release");
    d_states.release();
    *this = RayStore();
}
int RayStore::raycast(hipStream_t s, OccStore&, const lv_ray_params&, const void*, size_t, const void*, size_t, size_t, lv_ray_result*) {
    if (int rc = ran("RayStore::raycast", s)) return rc;
    if (int ra = d_states.need(4)) return ra;
    packed = true;
    return LV_OK;
}
int RayStore::view_gain(hipStream_t s, OccStore&, const lv_view*, size_t, uint64_t*) {
    if (int rc = ran("RayStore::view_gain", s)) return rc;
    if (int ra = d_states.need(4)) return ra;
    packed = true;
    return LV_OK;
}

// ---- lv_rollout.hip, lv_mcl.hip
void RolloutStore::release() {   // RolloutStore::release
    emu_hip::call("RolloutStore::release");
    d_res.release();
    *this = RolloutStore();
}
int RolloutStore::run(hipStream_t s, const PlanStore&, const DistStore&, const lv_rollout_params&, const float*, const float*, size_t, const float*, size_t,
                      lv_rollout_result*, float*, uint64_t*, int64_t*) {
    if (int rc = ran("RolloutStore::run", s)) return rc;
    return d_res.need(1);
}
void MclStore::release() {   // MclStore::release
    emu_hip::call("MclStore::release");
    d_score.release();
    *this = MclStore();
}
int MclStore::run(hipStream_t s, const DistStore&, const lv_mcl_params&, const float*, size_t, const float*, size_t, const uint32_t*, size_t, uint64_t*,
                  uint32_t*, int64_t*) {
    if (int rc = ran("MclStore::run", s)) return rc;
    return d_score.need(1);
}

// ---- lv_tsdf.hip
void TsdfStore::mesh_release() {   // TsdfStore::mesh_release
    emu_hip::call("TsdfStore::mesh_release");
    mesh.d_xyz.release();
    mesh = TsdfMesh();
}
void TsdfStore::release() {   // TsdfStore::release
    emu_hip::call("TsdfStore::release");
    mesh_release();
    d_S.release();
    *this = TsdfStore();
}
int TsdfStore::configure(hipStream_t s, const lv_tsdf_params& p) {   // TsdfStore::configure: release(), the shape, configured = true last
    if (int rc = ran("TsdfStore::configure", s)) return rc;
    release();
    prm = p;
    grid = tsdf_grid_of(p);
    for (int a = 0; a < 3; ++a) origin0[a] = p.origin[a];
    n_vox = grid_cells(grid.occ);
    if (int rc = d_S.need(n_vox)) return rc;
    configured = true;
    return LV_OK;
}
int TsdfStore::clear(hipStream_t s) { return ran("TsdfStore::clear", s); }
int TsdfStore::integrate(hipStream_t s, const lv_view*, size_t, uint64_t*) { return ran("TsdfStore::integrate", s); }
int TsdfStore::query(hipStream_t s, const void*, size_t, size_t, float*, int32_t*) { return ran("TsdfStore::query", s); }
int TsdfStore::fetch(hipStream_t s, int32_t*, int32_t*, float*) { return ran("TsdfStore::fetch", s); }
int TsdfStore::load(hipStream_t s, const int32_t*, const int32_t*) { return ran("TsdfStore::load", s); }
int TsdfStore::recentre(hipStream_t s, const int32_t*, const int32_t s_new[3], const float origin_new[3], uint64_t out[4]) {
    if (int rc = ran("TsdfStore::recentre", s)) return rc;
    if (out) { out[0] = n_vox - 1; out[1] = 1; out[2] = 1; out[3] = 0; }
    for (int a = 0; a < 3; ++a) {   // TsdfStore::recentre's last loop
        shift[a] = s_new[a];
        prm.origin[a] = origin_new[a];
        grid.occ.origin[a] = origin_new[a];
    }
    return LV_OK;
}
int TsdfStore::mesh_build(hipStream_t s, int min_weight, uint64_t*) {   // TsdfStore::mesh_build: mesh_release() first, the mesh's fields last
    const int rc = ran("TsdfStore::mesh_build", s);
    mesh_release();
    if (rc) return rc;
    if (int ra = mesh.d_xyz.need(15)) return ra;
    mesh.built = true;
    mesh.stale = 0;
    mesh.min_weight = min_weight;
    mesh.counts[0] = 5;
    mesh.counts[1] = 4;
    mesh.counts[2] = 5;
    mesh.counts[3] = 0;
    return LV_OK;
}
int TsdfStore::mesh_fetch(hipStream_t s, float*, int32_t*, uint32_t*) { return ran("TsdfStore::mesh_fetch", s); }

namespace {

using Calls = std::vector<std::string>;
// what ran since `from`: the stores' functions and the stream's calls (allocations are counted, not listed)
Calls calls(size_t from) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i)
        if (log[i].call != "hipMalloc" && log[i].call != "hipFree" && log[i].call != "hipHostMalloc" && log[i].call != "hipHostFree") v.push_back(log[i].call);
    return v;
}
size_t mark() { return emu_hip::state().log.size(); }
long live() { return emu_hip::state().mallocs - emu_hip::state().frees; }

std::string fmt(const char* f, ...) {
    char b[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof(b), f, ap);
    va_end(ap);
    return b;
}
// the call was refused with this code and exactly this message
#define REFUSED(call, code, msg)                          \
    do {                                                  \
        g_err[0] = 0;                                     \
        CHECK((call) == (code) && std::string(g_err) == (msg)); \
    } while (0)

// ---- today's messages (copied from lv_api.hip as it stood before the rules moved)
const char* const NO_GRID = "no occupancy grid: call lv_occ_configure first";
const char* const NO_FIELD = "no distance field: call lv_occ_distance_build first";
const char* const NO_PLAN = "no plan: call lv_occ_plan_build first";
const char* const NO_FRONTIER = "no frontier: call lv_occ_frontier_build first";
const char* const NO_SURFACE = "no TSDF volume: call lv_tsdf_configure first";
const char* const NO_MESH = "no mesh: call lv_tsdf_mesh_build first";
const char* const RANK_SHAPES = "lv_occ_frontier_rank: the plan (%d x %d x %d, planar %d) is not of the frontier's cells (%d x %d x %d, planar %d)";
const char* const RANK_SHIFTS = "lv_occ_frontier_rank: the frontier was built at grid shift (%d, %d, %d), the plan at (%d, %d, %d), the grid is at (%d, %d, %d): "
                                "rebuild the field, the plan and the frontier";
const char* const ROLL_3D = "lv_occ_rollout: the plan is 3-D: rollouts run on a planar plan";
const char* const ROLL_FIELD = "lv_occ_rollout: the distance field (%d x %d, planar %d) is not of the plan's cells (%d x %d, planar)";

const int NX = 8, NY = 8, NZ = 4;
const size_t NVOX = (size_t)NX * NY * NZ;

// a context's volume side as lv_api.hip holds it, with arguments every call accepts
struct Ctx {
    VolumeTools v;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    lv_view view{};
    uint8_t cost[2] = {1, 1};
    float goal[3] = {0.f, 0.f, 0.f}, start[3] = {0.f, 0.f, 0.f}, fp[2] = {0.f, 0.f};
    uint64_t st[4] = {0, 0, 0, 0};
    Ctx() { view.R[0] = view.R[4] = view.R[8] = 1.f; }
    ~Ctx() { v.release(); }

    int configure() {
        lv_occupancy_params p;
        default_occupancy_params(&p);
        p.nx = NX; p.ny = NY; p.nz = NZ;
        return v.occ_configure(s, p);
    }
    int surface() {
        lv_tsdf_params p;
        default_tsdf_params(&p);
        p.nx = NX; p.ny = NY; p.nz = NZ;
        return v.tsdf_configure(s, p);
    }
    int integrate() { return v.occ_integrate(s, &view, 1, st); }
    int field(bool planar) {
        lv_distance_params p;
        default_distance_params(&p);
        p.planar = planar;
        return v.distance_build(s, p, st);
    }
    int plan(bool planar) {
        lv_plan_params p;
        default_plan_params(&p);
        p.connectivity = planar ? 8 : 26;
        return v.plan_build(s, p, cost, 2, goal, 12, 1, st);
    }
    int frontier(bool planar) {
        lv_frontier_params p;
        default_frontier_params(&p);
        p.planar = planar;
        p.connectivity = planar ? 8 : 26;
        return v.frontier_build(s, p, st);
    }
    int chain(bool planar) {
        int rc = integrate();
        if (!rc) rc = field(planar);
        if (!rc) rc = plan(planar);
        if (!rc) rc = frontier(planar);
        return rc;
    }
    int raycast() {
        lv_ray_params p;
        default_ray_params(&p);
        lv_ray_result r;
        return v.raycast(s, p, start, 12, goal, 12, 1, &r);
    }
    int rollout(size_t n_fp) {
        lv_rollout_params p;
        default_rollout_params(&p);
        int64_t best[2];
        return v.rollout_run(s, p, start, nullptr, 0, n_fp ? fp : nullptr, n_fp, nullptr, nullptr, nullptr, best);
    }
    int mcl() {
        lv_mcl_params p;
        default_mcl_params(&p);
        const uint32_t table[1] = {0};
        int64_t best[2];
        return v.mcl_weigh(s, p, nullptr, 0, start, 1, table, 1, nullptr, nullptr, best);
    }
    int rank() {
        uint32_t best_p[3];
        return v.frontier_rank(s, 1, best_p, nullptr, 3);
    }
    int recentre(int volume, int dx, int dy, int dz) {
        const int32_t d[3] = {dx, dy, dz};
        return v.recentre(s, volume, d, st);
    }
    int mark_all() {   // lv_occ_mark with the caller's points, as lv_api.hip drives the two halves
        lv_occ_mark_params p;
        default_occ_mark_params(&p);
        int lo[3], hi[3];
        bool any = false;
        if (int rc = v.occ_mark_box(p, lo, hi, st, &any)) return rc;
        if (!any) return LV_OK;
        return v.occ_mark(s, p, lo, hi, nullptr, 0, start, 12, 1, st);
    }
    // the three snapshots' `stale` as the info calls report it (-1: not built)
    struct Stale { int field, plan, frontier; bool operator==(const Stale& o) const { return field == o.field && plan == o.plan && frontier == o.frontier; } };
    Stale stale() {
        lv_distance_info d;
        lv_plan_info p;
        lv_frontier_info f;
        CHECK(v.distance_info(&d) == LV_OK && v.plan_info(&p) == LV_OK && v.frontier_info(&f) == LV_OK);
        return {d.built ? d.stale : -1, p.built ? p.stale : -1, f.built ? f.stale : -1};
    }
    int mesh_stale() {
        lv_mesh_info m;
        CHECK(v.mesh_info(&m) == LV_OK);
        return m.built ? m.stale : -1;
    }
    lv_volume_shifts shifts() {
        lv_volume_shifts o;
        std::memset(&o, 0xff, sizeof(o));
        v.shift_info(&o);
        return o;
    }
};
bool is(const int32_t v[3], int x, int y, int z) { return v[0] == x && v[1] == y && v[2] == z; }

// ---- scenarios
void unconfigured() {
    Ctx c;
    VolumeTools& v = c.v;
    hipStream_t s = c.s;
    int lo[3], hi[3];
    bool any = false;
    lv_occ_mark_params mp;
    default_occ_mark_params(&mp);
    lv_distance_params dp{};
    lv_plan_params pp{};
    lv_frontier_params fp{};
    lv_ray_params rp{};
    lv_rollout_params op{};
    lv_mcl_params lp{};
    const int32_t d[3] = {1, 0, 0};
    size_t n = 0;
    const size_t t = mark();
    // every call that needs the grid names the grid, whatever else it would ask for after it (a field, a plan, a frontier)
#define NEEDS_GRID(call) REFUSED(call, LV_ESTATE, NO_GRID)
    NEEDS_GRID(v.occ_integrate(s, &c.view, 1, c.st));
    NEEDS_GRID(v.occ_query(s, nullptr, 0, 0, nullptr));
    NEEDS_GRID(v.occ_project(s, 0, 0, nullptr, 0));
    NEEDS_GRID(v.occ_fetch(s, nullptr, 0));
    NEEDS_GRID(v.occ_load(s, nullptr, 0));
    NEEDS_GRID(v.occ_clear(s));
    NEEDS_GRID(v.occ_get_params(nullptr));
    NEEDS_GRID(v.occ_mark_box(mp, lo, hi, c.st, &any));
    NEEDS_GRID(v.distance_build(s, dp, c.st));
    NEEDS_GRID(v.distance_build_cells(s, dp, nullptr, 0, c.st));
    NEEDS_GRID(v.distance_fetch(s, nullptr, nullptr, 0));
    NEEDS_GRID(v.distance_query(s, nullptr, 0, 0, nullptr, nullptr));
    NEEDS_GRID(v.distance_info(nullptr));
    NEEDS_GRID(v.distance_clear(s));
    NEEDS_GRID(v.plan_build(s, pp, c.cost, 2, c.goal, 12, 1, c.st));
    NEEDS_GRID(v.plan_fetch(s, nullptr, nullptr, 0));
    NEEDS_GRID(v.plan_paths(s, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
    NEEDS_GRID(v.plan_info(nullptr));
    NEEDS_GRID(v.plan_clear(s));
    NEEDS_GRID(v.frontier_build(s, fp, c.st));
    NEEDS_GRID(v.frontier_fetch(s, nullptr, 0));
    NEEDS_GRID(v.frontier_clusters(s, nullptr, 0, &n));
    NEEDS_GRID(v.frontier_rank(s, 0, nullptr, nullptr, 0));
    NEEDS_GRID(v.frontier_info(nullptr));
    NEEDS_GRID(v.frontier_clear(s));
    NEEDS_GRID(v.raycast(s, rp, nullptr, 0, nullptr, 0, 0, nullptr));
    NEEDS_GRID(v.view_gain(s, &c.view, 1, c.st));
    NEEDS_GRID(v.rollout_run(s, op, c.start, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    NEEDS_GRID(v.rollout_run(s, op, c.start, nullptr, 0, c.fp, 1, nullptr, nullptr, nullptr, nullptr));
    NEEDS_GRID(v.mcl_weigh(s, lp, nullptr, 0, c.start, 1, nullptr, 1, nullptr, nullptr, nullptr));
    NEEDS_GRID(v.recentre(s, LV_VOLUME_OCC, d, c.st));
#undef NEEDS_GRID
    // ... and every call that needs the volume the volume, before the mesh
#define NEEDS_SURFACE(call) REFUSED(call, LV_ESTATE, NO_SURFACE)
    NEEDS_SURFACE(v.tsdf_integrate(s, &c.view, 1, c.st));
    NEEDS_SURFACE(v.tsdf_query(s, nullptr, 0, 0, nullptr, nullptr));
    NEEDS_SURFACE(v.tsdf_fetch(s, nullptr, nullptr, nullptr, 0));
    NEEDS_SURFACE(v.tsdf_load(s, nullptr, nullptr, 0));
    NEEDS_SURFACE(v.tsdf_clear(s));
    NEEDS_SURFACE(v.tsdf_get_params(nullptr));
    NEEDS_SURFACE(v.mesh_build(s, 0, c.st));
    NEEDS_SURFACE(v.mesh_fetch(s, nullptr, nullptr, nullptr, 0, 0));
    NEEDS_SURFACE(v.mesh_info(nullptr));
    NEEDS_SURFACE(v.mesh_clear(s));
    NEEDS_SURFACE(v.recentre(s, LV_VOLUME_SURFACE, d, c.st));
#undef NEEDS_SURFACE
    CHECK(mark() == t);   // neither a store's function nor a HIP call
    // each volume stands alone: the grid alone does not serve the surface's calls, nor the surface the grid's
    CHECK(c.configure() == LV_OK);
    REFUSED(v.tsdf_clear(s), LV_ESTATE, NO_SURFACE);
    REFUSED(v.recentre(s, LV_VOLUME_SURFACE, d, c.st), LV_ESTATE, NO_SURFACE);
}

void chain() {
    Ctx c;
    CHECK(c.configure() == LV_OK);
    CHECK(c.recentre(LV_VOLUME_OCC, 1, 2, -1) == LV_OK);   // (so that a stamped shift is not the zeros of a fresh store)
    CHECK((c.stale() == Ctx::Stale{-1, -1, -1}));
    CHECK(c.chain(false) == LV_OK && c.raycast() == LV_OK);
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}) && c.v.ray.packed);
    lv_distance_info di;
    lv_plan_info pi;
    lv_frontier_info fi;
    CHECK(c.v.distance_info(&di) == LV_OK && di.built == 1 && di.planar == 0 && di.nx == NX && di.ny == NY && di.nz == NZ);
    CHECK(c.v.plan_info(&pi) == LV_OK && pi.built == 1 && pi.rounds == 1 && pi.params.connectivity == 26 && pi.nz == NZ);
    CHECK(c.v.frontier_info(&fi) == LV_OK && fi.built == 1 && fi.n_clusters == 3 && fi.params.connectivity == 26);
    lv_volume_shifts sh = c.shifts();
    CHECK(is(sh.grid, 1, 2, -1) && is(sh.field, 1, 2, -1) && is(sh.plan, 1, 2, -1) && is(sh.frontier, 1, 2, -1) && is(sh.surface, 0, 0, 0));
    CHECK(c.rank() == LV_OK);
    // a grid edit: the field and the frontier no longer show the grid, the packed states are dropped; the plan shows the FIELD
    CHECK(c.integrate() == LV_OK);
    CHECK((c.stale() == Ctx::Stale{1, 0, 1}) && !c.v.ray.packed);
    // a field edit: the plan no longer shows the field
    CHECK(c.field(false) == LV_OK);
    CHECK((c.stale() == Ctx::Stale{0, 1, 1}));
    CHECK(c.plan(false) == LV_OK && c.frontier(false) == LV_OK);
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}));
    // the other grid edits
    CHECK(c.raycast() == LV_OK && c.v.occ_clear(c.s) == LV_OK);
    CHECK((c.stale() == Ctx::Stale{1, 0, 1}) && !c.v.ray.packed);
    CHECK(c.field(false) == LV_OK && c.plan(false) == LV_OK && c.frontier(false) == LV_OK && c.raycast() == LV_OK);
    std::vector<float> L(NVOX, 0.f);
    CHECK(c.v.occ_load(c.s, L.data(), NVOX) == LV_OK);
    CHECK((c.stale() == Ctx::Stale{1, 0, 1}) && !c.v.ray.packed);
    // a refused load has edited nothing
    CHECK(c.field(false) == LV_OK && c.frontier(false) == LV_OK && c.raycast() == LV_OK);
    L[5] = 1000.f;
    CHECK(c.v.occ_load(c.s, L.data(), NVOX) == LV_EINVAL && std::strstr(g_err, "lv_occ_load: value 1000 at 5 outside"));
    CHECK((c.stale() == Ctx::Stale{0, 1, 0}) && c.v.ray.packed);
    // the field over the caller's cells is a field edit too, after its plane-size check
    CHECK(c.plan(false) == LV_OK);
    lv_distance_params dp{};
    dp.planar = 1;
    const std::vector<int8_t> cells((size_t)NX * NY, 0);
    REFUSED(c.v.distance_build_cells(c.s, dp, cells.data(), 5, c.st), LV_EINVAL, fmt("lv_occ_distance_build_cells: %zu cells for a plane of nx * ny = %zu", (size_t)5, (size_t)NX * NY));
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}));
    CHECK(c.v.distance_build_cells(c.s, dp, cells.data(), cells.size(), c.st) == LV_OK);
    CHECK((c.stale() == Ctx::Stale{0, 1, 0}));
}

void failures() {
    Ctx c;
    CHECK(c.configure() == LV_OK && c.chain(false) == LV_OK && c.raycast() == LV_OK);
    // the edit is recorded before the store's call, whatever that returns
    g_rc["OccStore::integrate"] = LV_EHIP;
    CHECK(c.integrate() == LV_EHIP);
    CHECK((c.stale() == Ctx::Stale{1, 0, 1}) && !c.v.ray.packed);
    g_rc.clear();
    CHECK(c.chain(false) == LV_OK && c.raycast() == LV_OK);
    // a failed recentre has moved nothing
    g_rc["OccStore::recentre"] = LV_EHIP;
    CHECK(c.recentre(LV_VOLUME_OCC, 1, 0, 0) == LV_EHIP);
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}) && c.v.ray.packed && is(c.shifts().grid, 0, 0, 0));
    g_rc.clear();
    // a mark that wrote no voxel, and one that failed, have edited nothing; one that wrote has
    g_marked = 0;
    CHECK(c.mark_all() == LV_OK && c.st[0] == 11 && c.st[1] == 7 && c.st[2] == 0 && c.st[3] == 2);
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}) && c.v.ray.packed);
    g_marked = 5;
    g_rc["OccStore::mark"] = LV_EHIP;
    CHECK(c.mark_all() == LV_EHIP);
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}) && c.v.ray.packed);
    g_rc.clear();
    CHECK(c.mark_all() == LV_OK && c.st[2] == 5);
    CHECK((c.stale() == Ctx::Stale{1, 0, 1}) && !c.v.ray.packed);
    // a failed field build stamps no shift, but the plan is stale already
    CHECK(c.chain(false) == LV_OK);
    CHECK(c.recentre(LV_VOLUME_OCC, 1, 0, 0) == LV_OK && is(c.v.occ.shift, 1, 0, 0));
    g_rc["DistStore::build"] = LV_EHIP;
    CHECK(c.field(false) == LV_EHIP);
    CHECK(is(c.v.dist.shift, 0, 0, 0) && c.v.plan.stale == 1);
    g_rc.clear();
    CHECK(c.field(false) == LV_OK && is(c.v.dist.shift, 1, 0, 0));
    // a failed plan or frontier build stamps none either
    g_rc["PlanStore::build"] = LV_EHIP;
    g_rc["FrontierStore::build"] = LV_EHIP;
    CHECK(c.plan(false) == LV_EHIP && is(c.v.plan.shift, 0, 0, 0));
    CHECK(c.frontier(false) == LV_EHIP && is(c.v.frontier.shift, 0, 0, 0));
    g_rc.clear();
    CHECK(c.plan(false) == LV_OK && is(c.v.plan.shift, 1, 0, 0));
    CHECK(c.frontier(false) == LV_OK && is(c.v.frontier.shift, 1, 0, 0));
    // the connectivity is judged against the field before the plan's build is entered
    const size_t t = mark();
    lv_plan_params pp;
    default_plan_params(&pp);   // 8: a planar field's
    REFUSED(c.v.plan_build(c.s, pp, c.cost, 2, c.goal, 12, 1, c.st), LV_EINVAL, "lv_occ_plan_build: connectivity: a 3-D field takes 6, 18 or 26");
    CHECK(calls(t).empty() && c.v.plan.built);
}

void recentre() {
    Ctx c;
    lv_volume_shifts sh = c.shifts();   // nothing configured: zeros
    CHECK(is(sh.grid, 0, 0, 0) && is(sh.surface, 0, 0, 0) && is(sh.field, 0, 0, 0) && is(sh.plan, 0, 0, 0) && is(sh.frontier, 0, 0, 0));
    CHECK(c.configure() == LV_OK && c.chain(false) == LV_OK && c.raycast() == LV_OK);
    // nothing moves: no store is called, nothing goes stale, the stats are zeros
    for (uint64_t& x : c.st) x = 9;
    size_t t = mark();
    CHECK(c.recentre(LV_VOLUME_OCC, 0, 0, 0) == LV_OK);
    CHECK(calls(t).empty() && c.st[0] == 0 && c.st[1] == 0 && c.st[2] == 0 && c.st[3] == 0);
    CHECK((c.stale() == Ctx::Stale{0, 0, 0}) && c.v.ray.packed && c.rank() == LV_OK);
    // the grid moves: a grid edit, and the snapshots lie in the old box until all three are rebuilt
    t = mark();
    CHECK(c.recentre(LV_VOLUME_OCC, 2, 0, -1) == LV_OK && c.st[0] == NVOX - 1 && c.st[1] == 1);
    CHECK(calls(t) == Calls{"OccStore::recentre"});
    CHECK((c.stale() == Ctx::Stale{1, 0, 1}) && !c.v.ray.packed);
    sh = c.shifts();
    CHECK(is(sh.grid, 2, 0, -1) && is(sh.field, 0, 0, 0) && is(sh.plan, 0, 0, 0) && is(sh.frontier, 0, 0, 0));
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHIFTS, 0, 0, 0, 0, 0, 0, 2, 0, -1));
    CHECK(c.field(false) == LV_OK);
    sh = c.shifts();
    CHECK(is(sh.grid, 2, 0, -1) && is(sh.field, 2, 0, -1) && is(sh.plan, 0, 0, 0) && is(sh.frontier, 0, 0, 0));
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHIFTS, 0, 0, 0, 0, 0, 0, 2, 0, -1));
    CHECK(c.plan(false) == LV_OK);
    sh = c.shifts();
    CHECK(is(sh.field, 2, 0, -1) && is(sh.plan, 2, 0, -1) && is(sh.frontier, 0, 0, 0));
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHIFTS, 0, 0, 0, 2, 0, -1, 2, 0, -1));
    CHECK(c.frontier(false) == LV_OK);
    sh = c.shifts();
    CHECK(is(sh.grid, 2, 0, -1) && is(sh.field, 2, 0, -1) && is(sh.plan, 2, 0, -1) && is(sh.frontier, 2, 0, -1));
    t = mark();
    CHECK(c.rank() == LV_OK && calls(t) == Calls{"FrontierStore::rank"});
    // a plan of an older field than the frontier's grid is refused the same way (the plan takes its FIELD's shift)
    CHECK(c.recentre(LV_VOLUME_OCC, -2, 0, 0) == LV_OK && c.frontier(false) == LV_OK);
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHIFTS, 0, 0, -1, 2, 0, -1, 0, 0, -1));
    CHECK(c.plan(false) == LV_OK);   // (of the field that still lies at 2, 0, -1)
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHIFTS, 0, 0, -1, 2, 0, -1, 0, 0, -1));
    // the limits of the accumulated shift are the rule's (lv_grid.hpp), reported under the entry point's name
    REFUSED(c.recentre(LV_VOLUME_OCC, 0, 0, -GRID_SHIFT_LIMIT), LV_EINVAL, "lv_volume_recentre: shift: the accumulated shift stays within +-2^20 voxels");
    // the surface moves: the mesh is stale, and nothing of the grid's is touched
    CHECK(c.field(false) == LV_OK && c.plan(false) == LV_OK && c.raycast() == LV_OK);
    CHECK(c.surface() == LV_OK && c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    const lv_volume_shifts before = c.shifts();
    for (uint64_t& x : c.st) x = 9;
    t = mark();
    CHECK(c.recentre(LV_VOLUME_SURFACE, 0, 0, 0) == LV_OK && calls(t).empty() && c.st[0] == 0 && c.mesh_stale() == 0);
    CHECK(c.recentre(LV_VOLUME_SURFACE, 0, 3, 0) == LV_OK && calls(t) == Calls{"TsdfStore::recentre"});
    CHECK(c.mesh_stale() == 1 && (c.stale() == Ctx::Stale{0, 0, 0}) && c.v.ray.packed);
    sh = c.shifts();
    CHECK(is(sh.surface, 0, 3, 0) && std::memcmp(sh.grid, before.grid, sizeof(sh.grid)) == 0 && std::memcmp(sh.field, before.field, sizeof(sh.field)) == 0 &&
          std::memcmp(sh.plan, before.plan, sizeof(sh.plan)) == 0 && std::memcmp(sh.frontier, before.frontier, sizeof(sh.frontier)) == 0);
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK);
    g_rc["TsdfStore::recentre"] = LV_EHIP;
    CHECK(c.recentre(LV_VOLUME_SURFACE, 1, 0, 0) == LV_EHIP && c.mesh_stale() == 0 && is(c.shifts().surface, 0, 3, 0));
    g_rc.clear();
}

void reconfigure() {
    Ctx c;
    CHECK(c.configure() == LV_OK && c.chain(true) == LV_OK && c.raycast() == LV_OK && c.rollout(0) == LV_OK && c.mcl() == LV_OK);
    CHECK(live() == 7);   // the grid and the six that belong to it hold one allocation each
    const size_t t = mark();
    CHECK(c.configure() == LV_OK);
    CHECK((calls(t) == Calls{"hipStreamSynchronize", "DistStore::release", "PlanStore::release", "FrontierStore::release", "RayStore::release",
                             "RolloutStore::release", "MclStore::release", "OccStore::configure", "OccStore::release"}));
    CHECK(emu_hip::state().log[t].call == "hipStreamSynchronize" && emu_hip::state().log[t].stream == c.s);   // (nothing is freed before it)
    CHECK(live() == 1 && c.v.occ.configured && !c.v.ray.packed);
    int32_t labels[1];
    uint32_t pot[1];
    float m[1];
    REFUSED(c.v.distance_fetch(c.s, nullptr, m, 1), LV_ESTATE, NO_FIELD);
    REFUSED(c.mcl(), LV_ESTATE, NO_FIELD);
    REFUSED(c.v.plan_fetch(c.s, pot, nullptr, 1), LV_ESTATE, NO_PLAN);
    REFUSED(c.rollout(0), LV_ESTATE, NO_PLAN);
    REFUSED(c.v.frontier_fetch(c.s, labels, 1), LV_ESTATE, NO_FRONTIER);
    REFUSED(c.rank(), LV_ESTATE, NO_FRONTIER);
    CHECK((c.stale() == Ctx::Stale{-1, -1, -1}));
    // the surface is a volume of its own: it outlives the grid's reconfiguration, and its own drops its mesh
    CHECK(c.surface() == LV_OK && c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.configure() == LV_OK);
    CHECK(c.v.tsdf.configured && c.mesh_stale() == 0 && live() == 3);
    CHECK(c.surface() == LV_OK && c.mesh_stale() == -1 && live() == 2);
}

void belong_together() {
    Ctx c;
    CHECK(c.configure() == LV_OK && c.chain(false) == LV_OK);
    size_t t = mark();
    REFUSED(c.rollout(0), LV_ESTATE, ROLL_3D);
    CHECK(c.chain(true) == LV_OK && c.rollout(0) == LV_OK && c.rollout(1) == LV_OK);
    // a footprint is held against the field: none, a 3-D one, one of another size
    CHECK(c.v.distance_clear(c.s) == LV_OK);
    CHECK(c.rollout(0) == LV_OK);   // (without a footprint the plan alone serves)
    t = mark();
    REFUSED(c.rollout(1), LV_ESTATE, NO_FIELD);
    REFUSED(c.mcl(), LV_ESTATE, NO_FIELD);
    CHECK(calls(t).empty());
    CHECK(c.field(false) == LV_OK);
    REFUSED(c.rollout(1), LV_ESTATE, fmt(ROLL_FIELD, NX, NY, 0, NX, NY));
    CHECK(c.field(true) == LV_OK && c.rollout(1) == LV_OK && c.mcl() == LV_OK);
    c.v.dist.grid.nx = NX + 1;   // (no call leaves a field of another size beside a plan: set by hand)
    REFUSED(c.rollout(1), LV_ESTATE, fmt(ROLL_FIELD, NX + 1, NY, 1, NX, NY));
    c.v.dist.grid.nx = NX;
    c.v.dist.grid.ny = NY - 1;
    REFUSED(c.rollout(1), LV_ESTATE, fmt(ROLL_FIELD, NX, NY - 1, 1, NX, NY));
    c.v.dist.grid.ny = NY;
    // the frontier's cells and the plan's: one shape
    CHECK(c.plan(true) == LV_OK && c.frontier(true) == LV_OK && c.rank() == LV_OK);
    CHECK(c.frontier(false) == LV_OK);
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHAPES, NX, NY, 1, 1, NX, NY, NZ, 0));
    CHECK(c.field(false) == LV_OK && c.plan(false) == LV_OK && c.frontier(true) == LV_OK);
    REFUSED(c.rank(), LV_ESTATE, fmt(RANK_SHAPES, NX, NY, NZ, 0, NX, NY, 1, 1));
    CHECK(c.frontier(false) == LV_OK && c.rank() == LV_OK);
    uint32_t best_p[3];
    REFUSED(c.v.frontier_rank(c.s, 1, best_p, nullptr, 2), LV_EINVAL, fmt("capacity %zu < %zu clusters", (size_t)2, (size_t)3));
    // what is missing is named in the entry point's order: the frontier before the plan, the plan before the field
    CHECK(c.v.plan_clear(c.s) == LV_OK);
    REFUSED(c.rank(), LV_ESTATE, NO_PLAN);
    REFUSED(c.rollout(1), LV_ESTATE, NO_PLAN);
    CHECK(c.v.frontier_clear(c.s) == LV_OK);
    REFUSED(c.rank(), LV_ESTATE, NO_FRONTIER);
}

void clears() {
    Ctx c;
    CHECK(c.configure() == LV_OK && c.chain(false) == LV_OK && c.surface() == LV_OK && c.v.mesh_build(c.s, 1, c.st) == LV_OK);
    size_t t = mark();
    CHECK(c.v.frontier_clear(c.s) == LV_OK && (calls(t) == Calls{"hipStreamSynchronize", "FrontierStore::release"}));
    CHECK((c.stale() == Ctx::Stale{0, 0, -1}));
    t = mark();
    CHECK(c.v.distance_clear(c.s) == LV_OK && (calls(t) == Calls{"hipStreamSynchronize", "DistStore::release"}));
    CHECK((c.stale() == Ctx::Stale{-1, 1, -1}));   // the plan's field is gone: a field edit
    t = mark();
    CHECK(c.v.plan_clear(c.s) == LV_OK && (calls(t) == Calls{"hipStreamSynchronize", "PlanStore::release"}));
    CHECK((c.stale() == Ctx::Stale{-1, -1, -1}));
    t = mark();
    CHECK(c.v.mesh_clear(c.s) == LV_OK && (calls(t) == Calls{"hipStreamSynchronize", "TsdfStore::mesh_release"}));
    CHECK(c.mesh_stale() == -1 && c.v.tsdf.configured);
    CHECK(live() == 2);   // the two volumes
    // clearing what is not there is the same call; a failed synchronise frees nothing
    CHECK(c.v.distance_clear(c.s) == LV_OK && c.field(false) == LV_OK);
    emu_hip::state().fail = [](const char* call) { return std::string(call) == "hipStreamSynchronize"; };
    t = mark();
    CHECK(c.v.distance_clear(c.s) == LV_EHIP && c.v.mesh_clear(c.s) == LV_EHIP && calls(t).empty() && c.v.dist.built);
    CHECK(c.configure() == LV_EHIP && calls(t).empty() && c.v.dist.built);
    emu_hip::state().fail = nullptr;
}

void surface() {
    Ctx c;
    CHECK(c.surface() == LV_OK);
    VolumeTools& v = c.v;
    float xyz[15];
    uint32_t tri[12];
    REFUSED(v.mesh_fetch(c.s, xyz, nullptr, tri, 5, 4), LV_ESTATE, NO_MESH);
    CHECK(v.tsdf_integrate(c.s, &c.view, 1, c.st) == LV_OK && c.mesh_stale() == -1);
    REFUSED(v.mesh_build(c.s, 0, c.st), LV_EINVAL, "lv_tsdf_mesh_build: min_weight = 0: at least 1");
    CHECK(v.mesh_build(c.s, 2, c.st) == LV_OK && c.mesh_stale() == 0);
    lv_mesh_info mi;
    CHECK(v.mesh_info(&mi) == LV_OK && mi.built == 1 && mi.min_weight == 2 && mi.vertices == 5 && mi.triangles == 4 && mi.active_cells == 5 && mi.refused_edges == 0);
    CHECK(v.tsdf_integrate(c.s, &c.view, 1, c.st) == LV_OK && c.mesh_stale() == 1);
    CHECK(v.mesh_build(c.s, 2, c.st) == LV_OK && c.mesh_stale() == 0);
    // a load that is refused has edited nothing
    std::vector<int32_t> S(NVOX, 0), W(NVOX, 0);
    REFUSED(v.tsdf_load(c.s, S.data(), W.data(), NVOX - 1), LV_EINVAL, fmt("lv_tsdf_load: %zu values for a volume of %zu voxels, or a null array", NVOX - 1, NVOX));
    W[7] = -1;
    REFUSED(v.tsdf_load(c.s, S.data(), W.data(), NVOX), LV_EINVAL, fmt("lv_tsdf_load: voxel %zu: S = %d, W = %d: 0 <= W <= max_weight and |S| <= T * W", (size_t)7, 0, -1));
    CHECK(c.mesh_stale() == 0);
    W[7] = 0;
    CHECK(v.tsdf_load(c.s, S.data(), W.data(), NVOX) == LV_OK && c.mesh_stale() == 1);
    CHECK(v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    CHECK(v.tsdf_clear(c.s) == LV_OK && c.mesh_stale() == 1);
    // (the edit is recorded before the store's call, as the grid's is)
    CHECK(v.mesh_build(c.s, 1, c.st) == LV_OK);
    g_rc["TsdfStore::integrate"] = LV_EHIP;
    CHECK(v.tsdf_integrate(c.s, &c.view, 1, c.st) == LV_EHIP && c.mesh_stale() == 1);
    g_rc.clear();
    CHECK(v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    // lv_tsdf_mesh_fetch: room for what is asked for, and only for that
    REFUSED(v.mesh_fetch(c.s, nullptr, nullptr, nullptr, 5, 4), LV_EINVAL, "lv_tsdf_mesh_fetch: xyz, sub and tri are all null");
    REFUSED(v.mesh_fetch(c.s, xyz, nullptr, tri, 4, 4), LV_EINVAL, "lv_tsdf_mesh_fetch: room for 5 vertices needed");
    int32_t sub[15];
    REFUSED(v.mesh_fetch(c.s, nullptr, sub, nullptr, 4, 4), LV_EINVAL, "lv_tsdf_mesh_fetch: room for 5 vertices needed");
    REFUSED(v.mesh_fetch(c.s, xyz, nullptr, tri, 5, 3), LV_EINVAL, "lv_tsdf_mesh_fetch: room for 4 triangles needed");
    const size_t t = mark();
    CHECK(v.mesh_fetch(c.s, xyz, nullptr, nullptr, 5, 0) == LV_OK && v.mesh_fetch(c.s, nullptr, nullptr, tri, 0, 4) == LV_OK);
    CHECK((calls(t) == Calls{"TsdfStore::mesh_fetch", "TsdfStore::mesh_fetch"}));
    // a failed mesh build leaves none
    g_rc["TsdfStore::mesh_build"] = LV_EHIP;
    CHECK(v.mesh_build(c.s, 1, c.st) == LV_EHIP && c.mesh_stale() == -1);
    g_rc.clear();
}

void argument_order() {
    Ctx c;
    VolumeTools& v = c.v;
    float out[1];
    // without a grid or a volume the state is what is wrong, whatever the arguments
    REFUSED(v.occ_integrate(c.s, nullptr, 0, c.st), LV_ESTATE, NO_GRID);
    REFUSED(v.occ_query(c.s, nullptr, 0, 1, nullptr), LV_ESTATE, NO_GRID);
    REFUSED(v.occ_load(c.s, nullptr, 0), LV_ESTATE, NO_GRID);
    REFUSED(v.tsdf_query(c.s, nullptr, 0, 1, nullptr, nullptr), LV_ESTATE, NO_SURFACE);
    // with one, the same arguments are
    CHECK(c.configure() == LV_OK && c.surface() == LV_OK && c.chain(false) == LV_OK);
    const size_t t = mark();
    REFUSED(v.occ_integrate(c.s, nullptr, 0, c.st), LV_EINVAL, "null argument");
    REFUSED(v.occ_integrate(c.s, &c.view, 0, c.st), LV_EINVAL, fmt("n_views = %zu: must be in 1..%d", (size_t)0, OCC_MAX_VIEWS));
    REFUSED(v.occ_integrate(c.s, &c.view, OCC_MAX_VIEWS + 1, c.st), LV_EINVAL, fmt("n_views = %zu: must be in 1..%d", (size_t)OCC_MAX_VIEWS + 1, OCC_MAX_VIEWS));
    lv_view bad = c.view;
    bad.R[3] = __builtin_nanf("");
    REFUSED(v.occ_integrate(c.s, &bad, 1, c.st), LV_EINVAL, "view 0: non-finite R");
    REFUSED(v.tsdf_integrate(c.s, &bad, 1, c.st), LV_EINVAL, "lv_tsdf_integrate: view 0: non-finite R");
    REFUSED(v.occ_query(c.s, nullptr, 0, 1, nullptr), LV_EINVAL, fmt("bad point array (stride %zu) or null output", (size_t)0));
    REFUSED(v.occ_query(c.s, c.start, 12, 0xFFFFFFF0ull / 4 + 1, out), LV_EINVAL, "too many points");
    REFUSED(v.occ_load(c.s, nullptr, 0), LV_EINVAL, fmt("lv_occ_load: %zu values for a grid of %zu voxels", (size_t)0, NVOX));
    REFUSED(v.tsdf_query(c.s, nullptr, 0, 1, nullptr, nullptr), LV_EINVAL, "lv_tsdf_query: metres and weight are both null");
    REFUSED(v.tsdf_query(c.s, nullptr, 0, 1, out, nullptr), LV_EINVAL, fmt("lv_tsdf_query: bad point array (stride %zu)", (size_t)0));
    // ... and a refused edit has edited nothing
    CHECK(calls(t).empty() && (c.stale() == Ctx::Stale{0, 0, 0}));
    // lv_occ_mark: the grid, then the box (an empty one ends the call with zero stats), then the mark
    lv_occ_mark_params mp;
    default_occ_mark_params(&mp);
    int lo[3], hi[3];
    bool any = true;
    mp.lo[0] = NX;
    for (uint64_t& x : c.st) x = 9;
    CHECK(v.occ_mark_box(mp, lo, hi, c.st, &any) == LV_OK && !any && c.st[0] == 0 && c.st[3] == 0);
    CHECK(v.occ_mark_box(mp, lo, hi, nullptr, &any) == LV_OK && !any);
    mp.lo[0] = 2;
    for (uint64_t& x : c.st) x = 9;
    CHECK(v.occ_mark_box(mp, lo, hi, c.st, &any) == LV_OK && any && c.st[0] == 9 && lo[0] == 2 && hi[0] == NX - 1 && lo[2] == 0 && hi[2] == NZ - 1);
    CHECK(calls(t).empty());
    // what the two integrates hand views_ok (lv_rules.hpp): their prefix, t not judged, and their own limit on the returns of one
    // view and of all together (the points of an over-long view are never read)
    const size_t occ_max = 0xFFFFFFF0ull / 4, tsdf_max = (size_t)1 << 24;
    lv_view two[2] = {c.view, c.view};
    two[0].points = two[1].points = c.start;
    two[0].stride = two[1].stride = 12;
    two[0].n = occ_max + 1;
    REFUSED(v.occ_integrate(c.s, two, 1, c.st), LV_EINVAL, "too many returns");
    two[0].n = occ_max;
    two[1].n = 1;
    REFUSED(v.occ_integrate(c.s, two, 2, c.st), LV_EINVAL, "too many returns");
    two[0].n = tsdf_max + 1;
    REFUSED(v.tsdf_integrate(c.s, two, 1, c.st), LV_EINVAL, "lv_tsdf_integrate: too many returns");
    two[0].n = tsdf_max;
    REFUSED(v.tsdf_integrate(c.s, two, 2, c.st), LV_EINVAL, "lv_tsdf_integrate: too many returns");
    CHECK(calls(t).empty());
    two[0].t[1] = __builtin_nanf("");        // (to the walks a view without evidence, OCC_T_LIMIT: not refused)
    two[1].t[2] = __builtin_huge_valf();
    two[1].n = 0;
    CHECK(v.tsdf_integrate(c.s, two, 2, c.st) == LV_OK);
    two[0].n = occ_max;
    CHECK(v.occ_integrate(c.s, two, 2, c.st) == LV_OK);
    CHECK((calls(t) == Calls{"TsdfStore::integrate", "OccStore::integrate"}));
}

void defaults() {
    lv_occupancy_params o;
    std::memset(&o, 0xff, sizeof(o));
    default_occupancy_params(&o);
    CHECK(o.origin[0] == -51.2f && o.origin[1] == -51.2f && o.origin[2] == -3.2f && o.resolution == 0.2f && o.nx == 512 && o.ny == 512 && o.nz == 64);
    CHECK(o.min_range == 1.f && o.max_range == 80.f && o.l_hit == 0.85f && o.l_miss == -0.4f && o.l_min == -2.f && o.l_max == 3.5f && o.l_occ == 0.4f &&
          o.l_free == -0.4f);
    CHECK(occ_check_params(&o) == nullptr);
    lv_distance_params d;
    std::memset(&d, 0xff, sizeof(d));
    default_distance_params(&d);
    CHECK(d.planar == 0 && d.k_lo == 0 && d.k_hi == 0 && d.unknown_is_obstacle == 0 && d.signed_field == 0 && d.max_cells == 0 && dist_check_params(&d) == nullptr);
    lv_plan_params p;
    std::memset(&p, 0xff, sizeof(p));
    default_plan_params(&p);
    CHECK(p.connectivity == 8 && p.min_clear_s2 == 1);
    lv_frontier_params f;
    std::memset(&f, 0xff, sizeof(f));
    default_frontier_params(&f);
    CHECK(f.planar == 0 && f.k_lo == 0 && f.k_hi == 0 && f.connectivity == 26 && f.min_size == 1 && fr_check_params(&f) == nullptr);
    lv_ray_params r;
    std::memset(&r, 0xff, sizeof(r));
    default_ray_params(&r);
    CHECK(r.stop_unknown == 0);
    lv_rollout_params ro;
    std::memset(&ro, 0xff, sizeof(ro));
    default_rollout_params(&ro);
    CHECK(ro.T == 32 && ro.Tc == 1 && ro.dt == 0.1f && ro.fp_clear_s2 == 1 && ro.w_cost == 1 && ro.w_goal == 1 && ro.w_stop == 0 && ro.min_steps == 1 &&
          ro.goal_mode == 0);
    lv_mcl_params m;
    std::memset(&m, 0xff, sizeof(m));
    default_mcl_params(&m);
    CHECK(m.out_cost == 0 && m.min_inside == 1);
    lv_tsdf_params t;
    std::memset(&t, 0xff, sizeof(t));
    default_tsdf_params(&t);   // (the occupancy grid's footprint)
    CHECK(t.origin[0] == -51.2f && t.origin[1] == -51.2f && t.origin[2] == -3.2f && t.resolution == 0.2f && t.nx == 512 && t.ny == 512 && t.nz == 64);
    CHECK(t.min_range == 1.f && t.max_range == 80.f && t.trunc_cells == 3 && t.max_weight == 10000 && t.carve == 0 && tsdf_check_params(&t) == nullptr);
    lv_occ_mark_params k;
    std::memset(&k, 0xff, sizeof(k));
    default_occ_mark_params(&k);
    for (int a = 0; a < 3; ++a) CHECK(k.lo[a] == 0 && k.hi[a] == (1 << 30));
    CHECK(k.min_points == 1 && k.only_unknown == 1 && k.l_mark == 0.85f);
    default_occupancy_params(nullptr);
    default_distance_params(nullptr);
    default_plan_params(nullptr);
    default_frontier_params(nullptr);
    default_ray_params(nullptr);
    default_rollout_params(nullptr);
    default_mcl_params(nullptr);
    default_tsdf_params(nullptr);
    default_occ_mark_params(nullptr);
}

void release() {
    VolumeTools v;
    {
        Ctx c;
        CHECK(c.configure() == LV_OK && c.chain(true) == LV_OK && c.raycast() == LV_OK && c.rollout(1) == LV_OK && c.mcl() == LV_OK);
        CHECK(c.surface() == LV_OK && c.v.mesh_build(c.s, 1, c.st) == LV_OK);
        CHECK(live() == 9);   // the two volumes, the mesh and the six that belong to the grid
        const size_t t = mark();
        c.v.release();
        // lv_destroy's order
        CHECK((calls(t) == Calls{"RayStore::release", "RolloutStore::release", "MclStore::release", "FrontierStore::release", "PlanStore::release",
                                 "DistStore::release", "OccStore::release", "TsdfStore::release", "TsdfStore::mesh_release"}));
        CHECK(live() == 0 && !c.v.occ.configured && !c.v.tsdf.configured && !c.v.dist.built && !c.v.plan.built && !c.v.frontier.built && !c.v.ray.packed);
        c.v.release();   // a second one is harmless
        CHECK(live() == 0);
        REFUSED(c.integrate(), LV_ESTATE, NO_GRID);
        CHECK(c.configure() == LV_OK && c.chain(false) == LV_OK);   // ... and the context's volume side starts over
    }
    CHECK(live() == 0);
    v.release();   // of tools that never held anything
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: volumes_emu <scenario>\n"); return 2; }
    const std::string s = argv[1];
    if (s == "unconfigured") unconfigured();
    else if (s == "chain") chain();
    else if (s == "failures") failures();
    else if (s == "recentre") recentre();
    else if (s == "reconfigure") reconfigure();
    else if (s == "belong_together") belong_together();
    else if (s == "clears") clears();
    else if (s == "surface") surface();
    else if (s == "argument_order") argument_order();
    else if (s == "defaults") defaults();
    else if (s == "release") release();
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees);
    printf("ok %s\n", s.c_str());
    return 0;
}
