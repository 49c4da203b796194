// tests/emu/surf_merge_state_emu.cpp — HOST test of lv_surf_merge's state rules in VolumeTools (limo-velo_amd/csrc/lv_volumes.hpp:
// surf_merge, its row of the stale table and its line of "WHAT A CALL ASKS FOR").
// TEST INFRASTRUCTURE ONLY: built by tests/test_surf_merge_state_host.py into tests/emu/_build/ (once plain, once with
// AddressSanitizer + UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own lv_volumes.hpp and tool headers,
// unchanged, against the stand-in hip_runtime.h next to this file, in the manner of surf_occ_state_emu.cpp, with its own stand-ins
// for the stores' member functions that its scenarios reach (volumes_emu.cpp stays as it is and knows nothing of this call).  The
// products are not built here: their `built` flags are set by hand, which is all the table reads.
// Usage: surf_merge_state_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>

#include "../../limo-velo_amd/csrc/lv_surf_merge.hpp"
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

uint64_t g_stats[4] = {0, 0, 0, 0};   // what merge hands back
int g_lo[3], g_hi[3];                 // the box it was given
int64_t g_kq = 0;                     // and the scale

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
    n_vox = grid_cells(grid);
    if (int rc = d_L.need(n_vox)) return rc;
    configured = true;
    return LV_OK;
}
void DistStore::release() { emu_hip::call("DistStore::release"); *this = DistStore(); }
void PlanStore::release() { emu_hip::call("PlanStore::release"); *this = PlanStore(); }
void FrontierStore::release() { emu_hip::call("FrontierStore::release"); *this = FrontierStore(); }
void RayStore::release() { emu_hip::call("RayStore::release"); *this = RayStore(); }
void RolloutStore::release() { emu_hip::call("RolloutStore::release"); *this = RolloutStore(); }
void MclStore::release() { emu_hip::call("MclStore::release"); *this = MclStore(); }
void TsdfStore::mesh_release() { emu_hip::call("TsdfStore::mesh_release"); mesh = TsdfMesh(); }
void TsdfStore::release() {
    emu_hip::call("TsdfStore::release");
    mesh_release();
    colour.release();
    *this = TsdfStore();
}
int TsdfStore::configure(hipStream_t s, const lv_tsdf_params& p) {
    if (int rc = ran("TsdfStore::configure", s)) return rc;
    prm = p;
    grid = tsdf_grid_of(p);
    n_vox = grid_cells(grid.occ);
    configured = true;
    return LV_OK;
}
int TsdfStore::merge(hipStream_t s, const lv_surf_submap&, const SurfMergeRule& q, const int lo[3], const int hi[3], uint64_t out[4]) {
    if (int rc = ran("TsdfStore::merge", s)) return rc;
    g_kq = q.kq;
    for (int a = 0; a < 3; ++a) {
        g_lo[a] = lo[a];
        g_hi[a] = hi[a];
    }
    if (out)
        for (int i = 0; i < 4; ++i) out[i] = g_stats[i];
    return LV_OK;
}

namespace {

using Calls = std::vector<std::string>;
Calls calls(size_t from) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i)
        if (log[i].call != "hipMalloc" && log[i].call != "hipFree" && log[i].call != "hipHostMalloc" && log[i].call != "hipHostFree") v.push_back(log[i].call);
    return v;
}
size_t mark() { return emu_hip::state().log.size(); }

#define REFUSED(call, code, msg)                          \
    do {                                                  \
        g_err[0] = 0;                                     \
        CHECK((call) == (code) && std::string(g_err) == (msg)); \
    } while (0)

const char* const NO_SURFACE = "no TSDF volume: call lv_tsdf_configure first";

const int NX = 24, NY = 20, NZ = 12;

struct Ctx {
    VolumeTools v;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    std::vector<int32_t> S, W;
    lv_surf_submap sub{};
    lv_graph_pose pose{};
    SurfMergeRule q;
    uint64_t st[4] = {7, 7, 7, 7};
    Ctx() : S(6 * 5 * 4, 0), W(6 * 5 * 4, 1) {
        sub.origin[0] = sub.origin[1] = sub.origin[2] = 0.5f;
        sub.resolution = 0.25f;
        sub.nx = 6; sub.ny = 5; sub.nz = 4;
        sub.trunc_cells = 3;
        sub.S = S.data();
        sub.W = W.data();
        pose.q[3] = 1.0;
        CHECK(rule() == LV_OK);
    }
    ~Ctx() { v.release(); }

    int rule() { return surf_merge_rule(&sub, &pose, nullptr, &q); }
    int surface(float resolution = 0.25f) {
        lv_tsdf_params p;
        default_tsdf_params(&p);
        p.origin[0] = p.origin[1] = p.origin[2] = 0.f;
        p.resolution = resolution;
        p.nx = NX; p.ny = NY; p.nz = NZ;
        return v.tsdf_configure(s, p);
    }
    int grid() {
        lv_occupancy_params p;
        default_occupancy_params(&p);
        p.nx = 8; p.ny = 6; p.nz = 4;
        return v.occ_configure(s, p);
    }
    int call(bool with_stats = true) {
        for (uint64_t& x : st) x = 7;
        return v.surf_merge(s, sub, q, with_stats ? st : nullptr);
    }
    // every product built, nothing stale, the packed states of both sides packed, a colour layer present
    void products() {
        v.dist.built = v.plan.built = v.frontier.built = v.lattice.built = v.tsdf.mesh.built = true;
        v.dist.stale = v.plan.stale = v.frontier.stale = v.lattice.stale = v.tsdf.mesh.stale = 0;
        v.ray.packed = true;
        v.tsdf.rays.packed = true;
        v.tsdf.colour.present = true;
    }
    bool surface_marked() const { return v.tsdf.mesh.stale == 1 && !v.tsdf.rays.packed; }
    bool surface_fresh() const { return v.tsdf.mesh.stale == 0 && v.tsdf.rays.packed; }
    bool others_untouched() const {
        return v.dist.stale == 0 && v.plan.stale == 0 && v.frontier.stale == 0 && v.lattice.stale == 0 && v.ray.packed && v.tsdf.colour.present;
    }
};

void set_stats(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    g_stats[0] = a; g_stats[1] = b; g_stats[2] = c; g_stats[3] = d;
}

// SURFACE, then the resolution ratio, then the store; the occupancy grid is never asked for
void order() {
    Ctx c;
    size_t t = mark();
    REFUSED(c.call(), LV_ESTATE, NO_SURFACE);
    CHECK(calls(t).empty() && c.st[0] == 7);
    CHECK(c.grid() == LV_OK);
    REFUSED(c.call(), LV_ESTATE, NO_SURFACE);   // (a grid does not help)
    c.v.occ.release();
    CHECK(c.surface(4.0f) == LV_OK);   // 0.25 into 4: a ratio of 1/16
    c.products();
    t = mark();
    REFUSED(c.call(), LV_EINVAL, "lv_surf_merge: the submap's resolution 0.25 against the volume's 4: a ratio of 1/8 to 8");
    CHECK(calls(t).empty() && c.st[0] == 7 && c.surface_fresh() && c.others_untouched());   // (refused: nothing marked)
    CHECK(c.surface(0.25f) == LV_OK);
    set_stats(3, 4, 5, 6);
    t = mark();
    CHECK(c.call() == LV_OK && (calls(t) == Calls{"TsdfStore::merge"}));
    CHECK(c.st[0] == 3 && c.st[1] == 4 && c.st[2] == 5 && c.st[3] == 6 && g_kq == 4096);
    // the submap's box 0.5 .. 2.0 x 0.5 .. 1.75 x 0.5 .. 1.5 m reaches the centres 0.125 + 0.25 i in it, widened by a voxel and a slack
    CHECK(g_lo[0] <= 2 && g_lo[0] >= 0 && g_hi[0] >= 8 && g_hi[0] <= 10 && g_lo[2] <= 2 && g_hi[2] >= 6 && g_hi[2] <= 8 && g_hi[1] >= 7 && g_hi[1] <= 9);
    CHECK(c.call(false) == LV_OK);   // stats may be NULL
    c.sub.resolution = 0.2f;         // 0.2 into 0.25: kq = floorf(0.8 * 4096 + 0.5)
    CHECK(c.rule() == LV_OK && c.call() == LV_OK && g_kq == 3277);
}

// once the arguments hold: mesh.stale = 1 where built, the surface rays' states not packed, whatever the store call returns; the
// colour layer, the occupancy side and its products are not touched
void marks() {
    Ctx c;
    CHECK(c.surface() == LV_OK && c.grid() == LV_OK);
    c.products();
    set_stats(9, 0, 0, 0);   // (nothing contributed: the marks do not depend on it)
    CHECK(c.call() == LV_OK && c.surface_marked() && c.others_untouched());
    c.products();
    CHECK(c.call(false) == LV_OK && c.surface_marked() && c.others_untouched());
    // a store call that fails
    c.products();
    g_rc["TsdfStore::merge"] = LV_EHIP;
    const size_t t = mark();
    CHECK(c.call() == LV_EHIP && c.surface_marked() && c.others_untouched() && c.st[0] == 7);
    CHECK(calls(t) == Calls{"TsdfStore::merge"});
    g_rc.clear();
    // a mesh that does not exist is not marked
    c.products();
    c.v.tsdf.mesh.built = false;
    CHECK(c.call() == LV_OK && c.v.tsdf.mesh.stale == 0 && !c.v.tsdf.rays.packed && c.others_untouched());
    // no occupancy grid at all: the call does not ask for one
    c.v.occ.release();
    CHECK(c.call() == LV_OK);
}

// a submap whose box cannot meet the volume: LV_OK, zero stats, no store call
void empty_box() {
    Ctx c;
    CHECK(c.surface() == LV_OK);
    c.products();
    set_stats(1, 1, 1, 1);
    const double away[3][3] = {{100.0, 0.0, 0.0}, {0.0, -30.0, 0.0}, {0.0, 0.0, 7.5}};
    for (const auto& t3 : away) {
        for (int a = 0; a < 3; ++a) c.pose.t[a] = t3[a];
        CHECK(c.rule() == LV_OK);
        const size_t t = mark();
        CHECK(c.call() == LV_OK && calls(t).empty());
        CHECK(c.st[0] == 0 && c.st[1] == 0 && c.st[2] == 0 && c.st[3] == 0);
        CHECK(c.others_untouched());
        CHECK(c.call(false) == LV_OK);
    }
    // ... but the states come before the box
    c.v.tsdf.release();
    REFUSED(c.call(), LV_ESTATE, NO_SURFACE);
    CHECK(c.st[0] == 7);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: surf_merge_state_emu <scenario>\n"); return 2; }
    const std::string s = argv[1];
    if (s == "order") order();
    else if (s == "marks") marks();
    else if (s == "empty_box") empty_box();
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees);
    printf("ok %s\n", s.c_str());
    return 0;
}
