// tests/emu/surf_occ_state_emu.cpp — HOST test of lv_occ_from_surface's state rules in VolumeTools (limo-velo_amd/csrc/lv_volumes.hpp:
// occ_from_surface, its row of the stale table and its line of "WHAT A CALL ASKS FOR").
// TEST INFRASTRUCTURE ONLY: built by tests/test_surf_occ_state_host.py into tests/emu/_build/ (once plain, once with
// AddressSanitizer + UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own lv_volumes.hpp and tool headers,
// unchanged, against the stand-in hip_runtime.h next to this file, in the manner of lattice_state_emu.cpp, with its own stand-ins for
// the stores' member functions that its scenarios reach (volumes_emu.cpp stays as it is and knows nothing of this call).  The products
// are not built here: their `built` flags are set by hand, which is all the table reads.
// Usage: surf_occ_state_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>

#include "../../limo-velo_amd/csrc/lv_surf_occ.hpp"
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

uint64_t g_stats[4] = {0, 0, 0, 0};   // what from_surface hands back
int g_lo[3], g_hi[3];                 // the box it was given
const TsdfStore* g_tsdf = nullptr;    // and the volume

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
int OccStore::from_surface(hipStream_t s, const TsdfStore& t, const lv_occ_surface_params&, const int lo[3], const int hi[3], uint64_t out[4]) {
    if (int rc = ran("OccStore::from_surface", s)) return rc;
    g_tsdf = &t;
    for (int a = 0; a < 3; ++a) {
        g_lo[a] = lo[a];
        g_hi[a] = hi[a];
    }
    for (int i = 0; i < 4; ++i) out[i] = g_stats[i];
    return LV_OK;
}
void DistStore::release() { emu_hip::call("DistStore::release"); *this = DistStore(); }
void PlanStore::release() { emu_hip::call("PlanStore::release"); *this = PlanStore(); }
void FrontierStore::release() { emu_hip::call("FrontierStore::release"); *this = FrontierStore(); }
void RayStore::release() { emu_hip::call("RayStore::release"); *this = RayStore(); }
void RolloutStore::release() { emu_hip::call("RolloutStore::release"); *this = RolloutStore(); }
void MclStore::release() { emu_hip::call("MclStore::release"); *this = MclStore(); }
void TsdfStore::mesh_release() { emu_hip::call("TsdfStore::mesh_release"); mesh = TsdfMesh(); }
void TsdfStore::release() { emu_hip::call("TsdfStore::release"); mesh_release(); *this = TsdfStore(); }
int TsdfStore::configure(hipStream_t s, const lv_tsdf_params& p) {
    if (int rc = ran("TsdfStore::configure", s)) return rc;
    prm = p;
    grid = tsdf_grid_of(p);
    n_vox = grid_cells(grid.occ);
    configured = true;
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

const char* const NO_GRID = "no occupancy grid: call lv_occ_configure first";
const char* const NO_SURFACE = "no TSDF volume: call lv_tsdf_configure first";

const int NX = 8, NY = 6, NZ = 4;

struct Ctx {
    VolumeTools v;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    lv_occ_surface_params p;
    uint64_t st[4] = {7, 7, 7, 7};
    Ctx() { default_occ_surface_params(&p); }
    ~Ctx() { v.release(); }

    int grid() {
        lv_occupancy_params q;
        default_occupancy_params(&q);
        q.nx = NX; q.ny = NY; q.nz = NZ;
        return v.occ_configure(s, q);
    }
    int surface() {
        lv_tsdf_params q;
        default_tsdf_params(&q);
        q.nx = 5; q.ny = 5; q.nz = 5;
        return v.tsdf_configure(s, q);
    }
    int call(bool with_stats = true) {
        for (uint64_t& x : st) x = 7;
        return v.occ_from_surface(s, p, with_stats ? st : nullptr);
    }
    // every product built, nothing stale, the rays' states packed
    void products() {
        v.dist.built = v.plan.built = v.frontier.built = v.lattice.built = v.tsdf.mesh.built = true;
        v.dist.stale = v.plan.stale = v.frontier.stale = v.lattice.stale = v.tsdf.mesh.stale = 0;
        v.ray.packed = true;
        v.tsdf.rays.packed = true;
    }
    bool grid_side_stale() const { return v.dist.stale == 1 && v.frontier.stale == 1 && !v.ray.packed; }
    bool grid_side_fresh() const { return v.dist.stale == 0 && v.frontier.stale == 0 && v.ray.packed; }
    bool others_untouched() const { return v.plan.stale == 0 && v.lattice.stale == 0 && v.tsdf.mesh.stale == 0 && v.tsdf.rays.packed; }
};

void set_stats(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    g_stats[0] = a; g_stats[1] = b; g_stats[2] = c; g_stats[3] = d;
}

// GRID, then SURFACE, then the box, then the store
void order() {
    Ctx c;
    size_t t = mark();
    REFUSED(c.call(), LV_ESTATE, NO_GRID);
    CHECK(c.surface() == LV_OK);
    REFUSED(c.call(), LV_ESTATE, NO_GRID);   // (the grid comes first whatever else is there)
    c.v.tsdf.release();
    CHECK(c.grid() == LV_OK);
    t = mark();
    REFUSED(c.call(), LV_ESTATE, NO_SURFACE);
    CHECK(calls(t).empty() && c.st[0] == 7);
    CHECK(c.surface() == LV_OK);
    set_stats(3, 4, 5, 6);
    t = mark();
    CHECK(c.call() == LV_OK && (calls(t) == Calls{"OccStore::from_surface"}));
    CHECK(c.st[0] == 3 && c.st[1] == 4 && c.st[2] == 5 && c.st[3] == 6 && g_tsdf == &c.v.tsdf);
    // the default box is the whole grid, clipped
    CHECK(g_lo[0] == 0 && g_lo[1] == 0 && g_lo[2] == 0 && g_hi[0] == NX - 1 && g_hi[1] == NY - 1 && g_hi[2] == NZ - 1);
    const int lo[3] = {-3, 2, 1}, hi[3] = {4, 99, 1};
    for (int a = 0; a < 3; ++a) {
        c.p.lo[a] = lo[a];
        c.p.hi[a] = hi[a];
    }
    CHECK(c.call() == LV_OK && g_lo[0] == 0 && g_lo[1] == 2 && g_lo[2] == 1 && g_hi[0] == 4 && g_hi[1] == NY - 1 && g_hi[2] == 1);
    CHECK(c.call(false) == LV_OK);   // stats may be NULL
}

// a box that is empty after clipping: LV_OK, zero stats, no store call, nothing marked
void empty_box() {
    Ctx c;
    CHECK(c.grid() == LV_OK && c.surface() == LV_OK);
    c.products();
    set_stats(1, 1, 1, 1);
    const int boxes[3][6] = {{NX, 0, 0, NX + 5, 9, 9}, {0, 3, 0, 9, 2, 9}, {0, 0, -9, 9, 9, -1}};
    for (const auto& b : boxes) {
        for (int a = 0; a < 3; ++a) {
            c.p.lo[a] = b[a];
            c.p.hi[a] = b[3 + a];
        }
        const size_t t = mark();
        CHECK(c.call() == LV_OK && calls(t).empty());
        CHECK(c.st[0] == 0 && c.st[1] == 0 && c.st[2] == 0 && c.st[3] == 0);
        CHECK(c.grid_side_fresh() && c.others_untouched());
        CHECK(c.call(false) == LV_OK);
    }
    // ... but the states come before the box
    c.v.tsdf.release();
    REFUSED(c.call(), LV_ESTATE, NO_SURFACE);
    CHECK(c.st[0] == 7);
}

// field and frontier go stale iff a voxel changed; plan, lattice and mesh never; a failing store call marks nothing
void stale() {
    Ctx c;
    CHECK(c.grid() == LV_OK && c.surface() == LV_OK);
    c.products();
    set_stats(10, 20, 0, 30);   // classed voxels, none changed
    CHECK(c.call() == LV_OK && c.st[0] == 10 && c.st[2] == 0 && c.grid_side_fresh() && c.others_untouched());
    set_stats(0, 0, 1, 0);
    CHECK(c.call() == LV_OK && c.grid_side_stale() && c.others_untouched());
    // without stats the rule is the same
    c.products();
    CHECK(c.call(false) == LV_OK && c.grid_side_stale() && c.others_untouched());
    c.products();
    set_stats(0, 0, 0, 0);
    CHECK(c.call(false) == LV_OK && c.grid_side_fresh());
    // a store call that fails
    set_stats(5, 5, 5, 5);
    g_rc["OccStore::from_surface"] = LV_EHIP;
    CHECK(c.call() == LV_EHIP && c.grid_side_fresh() && c.others_untouched() && c.st[0] == 7 && c.st[2] == 7);
    g_rc.clear();
    // products that do not exist are not marked
    c.v.dist.built = c.v.frontier.built = false;
    CHECK(c.call() == LV_OK && c.v.dist.stale == 0 && c.v.frontier.stale == 0 && !c.v.ray.packed && c.others_untouched());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: surf_occ_state_emu <scenario>\n"); return 2; }
    const std::string s = argv[1];
    if (s == "order") order();
    else if (s == "empty_box") empty_box();
    else if (s == "stale") stale();
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees);
    printf("ok %s\n", s.c_str());
    return 0;
}
