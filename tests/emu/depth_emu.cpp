// tests/emu/depth_emu.cpp — HOST test of the depth fusion (TEST INFRASTRUCTURE ONLY; g++ through tests/emu/hip/hip_runtime.h;
// built and run by tests/test_depth_host.py, never shipped).  Two halves:
//   depth_emu rule          the rule functions of limo-velo_amd/csrc/lv_depth.hpp on records read from stdin, one answer line per
//                           record; tests/test_depth_host.py holds them to tests/depth_ref.py.  Floats travel as their bits.  Records:
//                             u16 raw scale min_depth max_depth                 -> valid, D's bits
//                             f32 raw min_depth max_depth                       -> valid, D's bits
//                             quant D z resolution T carve                      -> adds, s
//                             unseen R[9] t[3] min max rho lo[3] hi[3]          -> 0 | 1 (depth_box_unseen)
//                             viewbox origin[3] res nx ny nz R[9] t[3] max rho  -> any lo[3] hi[3] (depth_view_box)
//                             rule <what> <value>                               -> ok ... | the refusal's message (depth_rule on one
//                                                                                  good view and the defaults with one thing changed)
//   depth_emu <scenario>    lv_depth_integrate's method of VolumeTools (lv_volumes.hpp) against stand-ins of TsdfStore's members
//                           that log themselves and return what the scenario set: the order of judgement, the SURFACE EDIT before the
//                           store call whatever it returns, and that the colour layer is not touched.  exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../../limo-velo_amd/csrc/lv_depth.hpp"
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

// ---- the stand-ins of lv_tsdf.hip, lv_colour.hip and lv_depth.hip (only what the scenarios reach)
void TsdfStore::mesh_release() {
    mesh.d_xyz.release();
    mesh = TsdfMesh();
}
void TsdfStore::release() {
    emu_hip::call("TsdfStore::release");
    mesh_release();
    d_S.release();
    colour.release();
    depth.release();
    *this = TsdfStore();
}
int TsdfStore::configure(hipStream_t s, const lv_tsdf_params& p) {
    if (int rc = ran("TsdfStore::configure", s)) return rc;
    release();
    prm = p;
    grid = tsdf_grid_of(p);
    n_vox = grid_cells(grid.occ);
    if (int rc = d_S.need(n_vox)) return rc;
    configured = true;
    return LV_OK;
}
int TsdfStore::mesh_build(hipStream_t s, int min_weight, uint64_t*) {
    const int rc = ran("TsdfStore::mesh_build", s);
    mesh_release();
    if (rc) return rc;
    if (int ra = mesh.d_xyz.need(15)) return ra;
    mesh.built = true;
    mesh.coloured = colour.present;
    mesh.stale = 0;
    mesh.min_weight = min_weight;
    return LV_OK;
}
int TsdfStore::colour_ensure(hipStream_t) {
    if (colour.present) return LV_OK;
    if (int rc = colour.d_sums.need(4 * n_vox)) return rc;
    colour.present = true;
    return LV_OK;
}
int TsdfStore::colour_load(hipStream_t s, const uint32_t*) {
    if (int rc = ran("TsdfStore::colour_load", s)) return rc;
    return colour_ensure(s);
}
int TsdfStore::integrate_depth(hipStream_t s, const lv_depth_view*, const DepthCam*, const DepthRule&, uint64_t*) {
    rays.packed = false;   // (the real one's first line)
    return ran("TsdfStore::integrate_depth", s);
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
long live() { return emu_hip::state().mallocs - emu_hip::state().frees; }

#define REFUSED(call, code, msg)                                \
    do {                                                        \
        g_err[0] = 0;                                           \
        CHECK((call) == (code) && std::string(g_err) == (msg)); \
    } while (0)

const char* const NO_SURFACE = "no TSDF volume: call lv_tsdf_configure first";

const int NX = 8, NY = 8, NZ = 4;
const size_t NVOX = (size_t)NX * NY * NZ;

struct Ctx {
    VolumeTools v;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    uint16_t pixels[6] = {1000, 1000, 1000, 1000, 1000, 1000};
    lv_depth_view view{};
    lv_depth_params prm{};
    DepthRule q{};
    DepthCam cams[DEPTH_MAX_VIEWS];
    uint64_t st[4] = {0, 0, 0, 0};
    Ctx() {
        view.R[0] = view.R[4] = view.R[8] = 1.f;
        view.fx = view.fy = 1.f;
        view.width = 3;
        view.height = 2;
        view.format = LV_DEPTH_U16;
        view.depth_scale = 0.001f;
        view.depth = pixels;
        view.row_stride = 6;
        default_depth_params(&prm);
    }
    ~Ctx() { v.tsdf.release(); }
    int surface() {
        lv_tsdf_params p;
        default_tsdf_params(&p);
        p.nx = NX; p.ny = NY; p.nz = NZ;
        return v.tsdf_configure(s, p);
    }
    // the entry point's two halves: the rule before the context, then the tools
    int integrate() {
        if (int rc = depth_rule(&view, 1, &prm, &q, cams)) return rc;
        return v.depth_integrate(s, &view, cams, q, st);
    }
    int mesh_stale() { return v.tsdf.mesh.built ? v.tsdf.mesh.stale : -1; }
};

void unconfigured() {
    Ctx c;
    const size_t t = mark();
    REFUSED(c.integrate(), LV_ESTATE, NO_SURFACE);
    CHECK(calls(t).empty() && live() == 0);
    // the arguments come before the volume: a rule that fails never reaches it
    c.prm.carve = 2;
    REFUSED(c.integrate(), LV_EINVAL, "lv_depth_integrate: carve = 2: 0 or 1");
    CHECK(calls(t).empty() && live() == 0);
}

void integrate() {
    Ctx c;
    CHECK(c.surface() == LV_OK);
    // without a mesh nothing goes stale; the store is called once
    size_t t = mark();
    CHECK(c.integrate() == LV_OK && (calls(t) == Calls{"TsdfStore::integrate_depth"}) && c.mesh_stale() == -1);
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    const long with_mesh = live();
    c.v.tsdf.rays.packed = true;
    t = mark();
    CHECK(c.integrate() == LV_OK && (calls(t) == Calls{"TsdfStore::integrate_depth"}));
    CHECK(c.mesh_stale() == 1 && !c.v.tsdf.rays.packed && live() == with_mesh);   // SURFACE EDIT; the stand-in allocates nothing
    lv_mesh_info mi;
    CHECK(c.v.mesh_info(&mi) == LV_OK && mi.built == 1 && mi.stale == 1);
    // the edit comes before the store call, whatever it returns
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    g_rc["TsdfStore::integrate_depth"] = LV_EHIP;
    CHECK(c.integrate() == LV_EHIP && c.mesh_stale() == 1);
    g_rc.clear();
    // a rule that fails marks nothing and calls nothing
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK);
    c.view.depth_scale = 0.f;
    t = mark();
    REFUSED(c.integrate(), LV_EINVAL, "lv_depth_integrate: view 0: depth_scale = 0: finite and > 0");
    CHECK(c.mesh_stale() == 0 && calls(t).empty());
}

void colour_untouched() {
    Ctx c;
    CHECK(c.surface() == LV_OK);
    std::vector<uint32_t> sums(4 * NVOX, 0u);
    CHECK(c.v.colour_load(c.s, sums.data(), NVOX) == LV_OK && c.v.tsdf.colour.present);
    uint32_t* const layer = c.v.tsdf.colour.d_sums.p;
    const long with_layer = live();
    const size_t t = mark();
    CHECK(c.integrate() == LV_OK && (calls(t) == Calls{"TsdfStore::integrate_depth"}));   // no colour member ran
    CHECK(c.v.tsdf.colour.present && c.v.tsdf.colour.d_sums.p == layer && live() == with_layer);
}

void defaults() {
    lv_depth_params p;
    default_depth_params(&p);
    CHECK(p.min_depth == 0.3f && p.max_depth == 10.f && p.max_norm_radius == 1.5f && p.carve == 0 && p.reserved == 0);
    lv_paint_params v;
    default_paint_params(&v);
    CHECK(p.min_depth == v.min_depth && p.max_norm_radius == v.max_norm_radius);
    default_depth_params(nullptr);
    // the record of a view: paint_project's fields from the pose and the intrinsics, the staged bytes back to back
    Ctx c;
    lv_depth_view two[2] = {c.view, c.view};
    two[1].format = LV_DEPTH_F32;
    two[1].row_stride = 12;
    two[1].dist[2] = 0.25f;
    CHECK(depth_rule(two, 2, &c.prm, &c.q, c.cams) == LV_OK);
    CHECK(c.q.view.n_views == 2 && c.q.view.min_depth == 0.3f && c.q.view.max_depth == 10.f && c.q.view.r2_max == 2.25f && c.q.rho == 1.5f && c.q.carve == 0);
    CHECK(c.cams[0].cam.raw_off == 0 && c.cams[1].cam.raw_off == 256 && c.q.raw_bytes == 512);
    CHECK(c.cams[0].cam.wm1 == 2.f && c.cams[0].cam.hm1 == 1.f && c.cams[0].cam.width == 3 && c.cams[0].cam.height == 2);
    CHECK(c.cams[0].scale == 0.001f && c.cams[1].scale == 1.f && c.cams[1].cam.format == LV_DEPTH_F32 && c.cams[1].cam.p1 == 0.25f && c.cams[0].cam.p1 == 0.f);
    // staging honours the stride: a padded image arrives packed
    uint16_t wide[8] = {1, 2, 3, 99, 4, 5, 6, 99};
    lv_depth_view pad = c.view;
    pad.depth = wide;
    pad.row_stride = 8;
    CHECK(depth_rule(&pad, 1, &c.prm, &c.q, c.cams) == LV_OK);
    std::vector<uint8_t> raw(c.q.raw_bytes, 0xEE);
    depth_stage_images(&pad, c.cams, 1, raw.data());
    const uint16_t* got = reinterpret_cast<const uint16_t*>(raw.data());
    CHECK(got[0] == 1 && got[1] == 2 && got[2] == 3 && got[3] == 4 && got[4] == 5 && got[5] == 6 && raw[12] == 0xEE);
}

float fbits(unsigned long long u) { return __uint_as_float((unsigned)u); }

int rule() {
    char op[32];
    while (scanf("%31s", op) == 1) {
        const std::string o = op;
        auto u = []() { unsigned long long v = 0; if (scanf("%llu", &v) != 1) exit(2); return v; };
        auto i = []() { long long v = 0; if (scanf("%lld", &v) != 1) exit(2); return v; };
        auto f = [&u]() { return fbits(u()); };
        if (o == "u16") {
            const uint16_t raw = (uint16_t)u();
            const float scale = f(), mn = f(), mx = f();
            float D = 0.f;
            const bool ok = depth_of_u16(raw, scale, mn, mx, D);
            printf("%d %u\n", ok ? 1 : 0, __float_as_uint(D));
        } else if (o == "f32") {
            const float raw = f(), mn = f(), mx = f();
            float D = 0.f;
            const bool ok = depth_of_f32(raw, mn, mx, D);
            printf("%d %u\n", ok ? 1 : 0, __float_as_uint(D));
        } else if (o == "quant") {
            const float D = f(), z = f(), res = f();
            const int32_t T = (int32_t)i();
            const int carve = (int)i();
            int32_t s = 0;
            const bool adds = depth_quant(D, z, res, T, carve, s);
            printf("%d %d\n", adds ? 1 : 0, adds ? s : 0);
        } else if (o == "unseen") {
            PaintCam c{};
            for (auto& x : c.R) x = f();
            for (auto& x : c.t) x = f();
            const float mn = f(), mx = f(), rho = f();
            float lo[3], hi[3];
            for (auto& x : lo) x = f();
            for (auto& x : hi) x = f();
            printf("%d\n", depth_box_unseen(c, mn, mx, rho, lo, hi) ? 1 : 0);
        } else if (o == "viewbox") {
            lv_tsdf_params p;
            default_tsdf_params(&p);
            for (auto& x : p.origin) x = f();
            p.resolution = f();
            p.nx = (int)i(); p.ny = (int)i(); p.nz = (int)i();
            const TsdfGrid g = tsdf_grid_of(p);
            PaintCam c{};
            for (auto& x : c.R) x = f();
            for (auto& x : c.t) x = f();
            const float mx = f(), rho = f();
            int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
            const bool any = depth_view_box(g, c, mx, rho, lo, hi);
            printf("%d %d %d %d %d %d %d\n", any ? 1 : 0, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
        } else if (o == "rule") {
            char what[32];
            if (scanf("%31s", what) != 1) return 2;
            const std::string w = what;
            const double val = [] { double v = 0; char b[64]; if (scanf("%63s", b) != 1) exit(2); const std::string s = b;
                                    if (s == "nan") return (double)std::numeric_limits<float>::quiet_NaN();
                                    if (s == "inf") return (double)std::numeric_limits<float>::infinity();
                                    sscanf(b, "%lf", &v); return v; }();
            Ctx c;
            std::vector<lv_depth_view> views(33, c.view);
            size_t n = 1;
            const lv_depth_view* vp = views.data();
            const lv_depth_params* pp = &c.prm;
            lv_depth_view& v0 = views[0];
            if (w == "ok") {}
            else if (w == "n_views") n = (size_t)val;
            else if (w == "views") vp = nullptr;
            else if (w == "params") pp = nullptr;
            else if (w == "min_depth") c.prm.min_depth = (float)val;
            else if (w == "max_depth") c.prm.max_depth = (float)val;
            else if (w == "max_norm_radius") c.prm.max_norm_radius = (float)val;
            else if (w == "carve") c.prm.carve = (int)val;
            else if (w == "R") v0.R[4] = (float)val;
            else if (w == "t") v0.t[1] = (float)val;
            else if (w == "fx") v0.fx = (float)val;
            else if (w == "cy") v0.cy = (float)val;
            else if (w == "dist") v0.dist[4] = (float)val;
            else if (w == "width") { v0.width = (int)val; v0.row_stride = 1 << 20; }
            else if (w == "height") v0.height = (int)val;
            else if (w == "side") { v0.width = v0.height = (int)val; v0.row_stride = 1 << 20; }
            else if (w == "format") v0.format = (int)val;
            else if (w == "depth_scale") v0.depth_scale = (float)val;
            else if (w == "depth") v0.depth = nullptr;
            else if (w == "row_stride") v0.row_stride = (size_t)val;
            else if (w == "f32_stride") { v0.format = LV_DEPTH_F32; v0.row_stride = (size_t)val; }
            else if (w == "f32_scale") { v0.format = LV_DEPTH_F32; v0.row_stride = 12; v0.depth_scale = (float)val; }
            else if (w == "total") {   // views of 4096 x 4096 = 2^24 pixels each
                n = (size_t)val;
                for (auto& x : views) { x.width = x.height = 4096; x.row_stride = 8192; }
            } else return 2;
            g_err[0] = 0;
            const int rc = depth_rule(vp, n, pp, &c.q, c.cams);
            if (rc == LV_OK) printf("ok %d %zu\n", c.q.view.n_views, c.q.raw_bytes);
            else printf("%s\n", g_err);
        } else {
            return 2;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "rule") return rule();
    const std::map<std::string, void (*)()> scenarios = {{"unconfigured", unconfigured}, {"integrate", integrate}, {"colour_untouched", colour_untouched},
                                                         {"defaults", defaults}};
    const auto it = scenarios.find(s);
    if (it == scenarios.end()) return 2;
    it->second();
    printf("ok %s\n", s.c_str());
    return 0;
}
