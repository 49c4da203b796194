// tests/emu/colour_emu.cpp — HOST test of the colour layer (TEST INFRASTRUCTURE ONLY; g++ through tests/emu/hip/hip_runtime.h;
// built and run by tests/test_colour_host.py, never shipped).  Two halves:
//   colour_emu rule          the rule functions of limo-velo_amd/csrc/lv_colour.hpp on records read from stdin, one answer line
//                            per record; tests/test_colour_host.py holds them to tests/colour_ref.py.  Records:
//                              cand S W min_weight band                      -> 0 | 1
//                              centre <origin bits> <resolution bits> i      -> the centre's bits
//                              quant <sample bits>                           -> the level
//                              fold max_weight n dC[3] C[3] Wc               -> C[3] Wc
//                              voxel C[3] Wc                                 -> r g b a
//                              vertex 8 x (C[3] Wc)                          -> r g b a
//                              layer n, then n x (C[3] Wc)                   -> the first voxel refused, or n
//                              params blend band min_weight max_weight       -> ok | the refusal's message
//   colour_emu <scenario>    the colour methods of VolumeTools (lv_volumes.hpp) against stand-ins of TsdfStore's members that log
//                            themselves and return what the scenario set: the order of judgement, the stale rows, and that
//                            nothing is allocated before the first lv_colour_integrate / lv_colour_load.  exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

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

// ---- the stand-ins of lv_tsdf.hip and lv_colour.hip (only what the colour methods and their scenarios reach)
void TsdfStore::mesh_release() {
    mesh.d_xyz.release();
    mesh.d_rgba.release();
    mesh = TsdfMesh();
}
void TsdfStore::release() {
    emu_hip::call("TsdfStore::release");
    mesh_release();
    d_S.release();
    colour.release();
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
int TsdfStore::mesh_build(hipStream_t s, int min_weight, uint64_t*) {   // the real one's last lines: coloured follows the layer
    const int rc = ran("TsdfStore::mesh_build", s);
    mesh_release();
    if (rc) return rc;
    if (int ra = mesh.d_xyz.need(15)) return ra;
    if (colour.present)
        if (int ra = mesh.d_rgba.need(5)) return ra;
    mesh.built = true;
    mesh.coloured = colour.present;
    mesh.stale = 0;
    mesh.min_weight = min_weight;
    mesh.counts[0] = 5;
    mesh.counts[1] = 4;
    mesh.counts[2] = 5;
    return LV_OK;
}
int TsdfStore::colour_ensure(hipStream_t) {
    if (colour.present) return LV_OK;
    if (int rc = colour.d_sums.need(4 * n_vox)) return rc;
    colour.present = true;
    return LV_OK;
}
int TsdfStore::colour_integrate(hipStream_t s, const lv_camera_view*, const PaintCam*, const PaintRule&, int, int, int, uint64_t*) {
    if (int rc = ran("TsdfStore::colour_integrate", s)) return rc;
    return colour_ensure(s);
}
int TsdfStore::colour_load(hipStream_t s, const uint32_t*) {
    if (int rc = ran("TsdfStore::colour_load", s)) return rc;
    return colour_ensure(s);
}
int TsdfStore::colour_fetch(hipStream_t s, uint32_t*, uint8_t*) { return ran("TsdfStore::colour_fetch", s); }
int TsdfStore::colour_query(hipStream_t s, const void*, size_t, size_t, uint8_t*) { return ran("TsdfStore::colour_query", s); }
int TsdfStore::colour_clear(hipStream_t s) { return ran("TsdfStore::colour_clear", s); }
int TsdfStore::colour_count(hipStream_t s, uint64_t* n) {
    *n = 42;
    return ran("TsdfStore::colour_count", s);
}
int TsdfStore::mesh_colours(hipStream_t s, uint8_t*) { return ran("TsdfStore::mesh_colours", s); }

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
const char* const NO_LAYER = "no colour layer: call lv_colour_integrate or lv_colour_load first";
const char* const NO_MESH = "no mesh: call lv_tsdf_mesh_build first";
const char* const GREY_MESH = "the mesh was built without a colour layer: call lv_tsdf_mesh_build after lv_colour_integrate";

const int NX = 8, NY = 8, NZ = 4;
const size_t NVOX = (size_t)NX * NY * NZ;

struct Ctx {
    VolumeTools v;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    uint8_t pixel[3] = {1, 2, 3};
    lv_camera_view view{};
    lv_colour_params prm{};
    PaintRule q{};
    PaintCam cams[PAINT_MAX_VIEWS];
    uint64_t st[4] = {0, 0, 0, 0};
    std::vector<uint32_t> sums = std::vector<uint32_t>(4 * NVOX, 0u);
    uint8_t rgba[64] = {0};
    Ctx() {
        view.R[0] = view.R[4] = view.R[8] = 1.f;
        view.fx = view.fy = 1.f;
        view.width = view.height = 1;
        view.image = pixel;
        view.row_stride = 3;
        default_colour_params(&prm);
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
        if (int rc = colour_rule(&view, 1, &prm, &q, cams)) return rc;
        return v.colour_integrate(s, &view, cams, q, prm, st);
    }
    int mesh_stale() { return v.tsdf.mesh.built ? v.tsdf.mesh.stale : -1; }
};

void unconfigured() {
    Ctx c;
    struct lv_colour_info info;
    const size_t t = mark();
    REFUSED(c.integrate(), LV_ESTATE, NO_SURFACE);
    REFUSED(c.v.colour_fetch(c.s, c.sums.data(), nullptr, NVOX), LV_ESTATE, NO_SURFACE);
    REFUSED(c.v.colour_load(c.s, c.sums.data(), NVOX), LV_ESTATE, NO_SURFACE);
    REFUSED(c.v.colour_query(c.s, nullptr, 0, 0, nullptr), LV_ESTATE, NO_SURFACE);
    REFUSED(c.v.colour_clear(c.s), LV_ESTATE, NO_SURFACE);
    REFUSED(c.v.colour_info(c.s, &info), LV_ESTATE, NO_SURFACE);
    REFUSED(c.v.mesh_colours(c.s, c.rgba, 16), LV_ESTATE, NO_SURFACE);
    CHECK(calls(t).empty() && live() == 0);
    // the arguments come before the volume: a rule that fails never reaches it
    c.prm.view.blend = 1;
    REFUSED(c.integrate(), LV_EINVAL, "lv_colour_integrate: blend = 1: the layer takes the mean, blend 0");
}

void no_layer() {
    Ctx c;
    struct lv_colour_info info;
    CHECK(c.surface() == LV_OK);
    const long base = live();
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    const long with_mesh = live();
    size_t t = mark();
    REFUSED(c.v.colour_fetch(c.s, c.sums.data(), nullptr, NVOX), LV_ESTATE, NO_LAYER);
    REFUSED(c.v.colour_fetch(c.s, c.sums.data(), nullptr, 0), LV_ESTATE, NO_LAYER);   // (the layer before the capacity)
    REFUSED(c.v.colour_query(c.s, nullptr, 0, 0, nullptr), LV_ESTATE, NO_LAYER);
    CHECK(c.v.colour_clear(c.s) == LV_OK && c.mesh_stale() == 0);   // LV_OK, nothing done, nothing stale
    CHECK(c.v.colour_info(c.s, &info) == LV_OK && info.present == 0 && info.voxels == NVOX && info.coloured == 0);
    REFUSED(c.v.mesh_colours(c.s, c.rgba, 16), LV_ESTATE, GREY_MESH);
    lv_mesh_info mi;
    CHECK(c.v.mesh_info(&mi) == LV_OK && mi.built == 1 && mi.reserved == 0);
    CHECK(calls(t).empty() && live() == with_mesh);   // nothing ran, nothing allocated
    CHECK(c.v.mesh_clear(c.s) == LV_OK && live() == base);
    REFUSED(c.v.mesh_colours(c.s, c.rgba, 16), LV_ESTATE, NO_MESH);
}

void integrate() {
    Ctx c;
    CHECK(c.surface() == LV_OK);
    const long base = live();
    // what is the call's own comes after the volume: band against T, nothing stale, nothing allocated
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK);
    const long with_mesh = live();
    c.prm.band = c.v.tsdf.grid.T + 1;
    size_t t = mark();
    REFUSED(c.integrate(), LV_EINVAL, "lv_colour_integrate: band = 769: must be in 1..T = 768");
    CHECK(calls(t).empty() && c.mesh_stale() == 0 && live() == with_mesh);
    c.prm.band = c.v.tsdf.grid.T;
    t = mark();
    CHECK(c.integrate() == LV_OK && (calls(t) == Calls{"TsdfStore::colour_integrate"}));
    CHECK(c.mesh_stale() == 1 && c.v.tsdf.colour.present && live() == with_mesh + 1);   // COLOUR EDIT; the layer is the one allocation
    lv_mesh_info mi;
    CHECK(c.v.mesh_info(&mi) == LV_OK && mi.reserved == 0 && mi.stale == 1);   // the mesh of before carries no colours
    REFUSED(c.v.mesh_colours(c.s, c.rgba, 16), LV_ESTATE, GREY_MESH);
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.v.mesh_info(&mi) == LV_OK && mi.reserved == 1 && mi.stale == 0);
    REFUSED(c.v.mesh_colours(c.s, c.rgba, 4), LV_EINVAL, "lv_mesh_colours: room for 5 vertices needed");
    t = mark();
    CHECK(c.v.mesh_colours(c.s, c.rgba, 5) == LV_OK && (calls(t) == Calls{"TsdfStore::mesh_colours"}));
    // the edit comes before the store call, whatever it returns
    g_rc["TsdfStore::colour_integrate"] = LV_EHIP;
    CHECK(c.integrate() == LV_EHIP && c.mesh_stale() == 1);
    g_rc.clear();
    // a rule that fails marks nothing
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK);
    c.prm.max_weight = 65536;
    REFUSED(c.integrate(), LV_EINVAL, "lv_colour_integrate: max_weight = 65536: must be in 1..65535");
    CHECK(c.mesh_stale() == 0);
    // lv_tsdf_configure frees the layer with everything else
    CHECK(c.surface() == LV_OK && !c.v.tsdf.colour.present && live() == base);
}

void load_clear() {
    Ctx c;
    struct lv_colour_info info;
    CHECK(c.surface() == LV_OK);
    const long base = live();
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK);
    REFUSED(c.v.colour_load(c.s, c.sums.data(), NVOX - 1), LV_EINVAL, "lv_colour_load: 255 voxels for a volume of 256");
    c.sums[4 * 7 + 1] = 256;
    c.sums[4 * 7 + 3] = 1;
    REFUSED(c.v.colour_load(c.s, c.sums.data(), NVOX), LV_EINVAL, "lv_colour_load: voxel 7: C = 0, 256, 0, Wc = 1: Wc <= 65535 and C <= 255 * Wc");
    CHECK(c.mesh_stale() == 0 && !c.v.tsdf.colour.present && live() == base + 1);   // refused: nothing stale, nothing allocated
    c.sums[4 * 7 + 1] = 255;
    size_t t = mark();
    CHECK(c.v.colour_load(c.s, c.sums.data(), NVOX) == LV_OK && (calls(t) == Calls{"TsdfStore::colour_load"}));
    CHECK(c.mesh_stale() == 1 && c.v.tsdf.colour.present && live() == base + 2);
    CHECK(c.v.colour_info(c.s, &info) == LV_OK && info.present == 1 && info.coloured == 42);
    REFUSED(c.v.colour_fetch(c.s, c.sums.data(), nullptr, NVOX - 1), LV_EINVAL, "lv_colour_fetch: room for nx * ny * nz = 256 voxels needed");
    t = mark();
    CHECK(c.v.colour_fetch(c.s, c.sums.data(), nullptr, NVOX) == LV_OK && c.v.colour_query(c.s, nullptr, 0, 0, nullptr) == LV_OK);
    CHECK((calls(t) == Calls{"TsdfStore::colour_fetch", "TsdfStore::colour_query"}));
    CHECK(c.v.mesh_build(c.s, 1, c.st) == LV_OK && c.mesh_stale() == 0);
    t = mark();
    CHECK(c.v.colour_clear(c.s) == LV_OK && (calls(t) == Calls{"TsdfStore::colour_clear"}));
    CHECK(c.mesh_stale() == 1 && c.v.tsdf.colour.present);   // zeroes, keeps the allocation
}

int rule() {
    char op[32];
    while (scanf("%31s", op) == 1) {
        const std::string o = op;
        auto u = []() { unsigned long long v = 0; if (scanf("%llu", &v) != 1) exit(2); return v; };
        auto i = []() { long long v = 0; if (scanf("%lld", &v) != 1) exit(2); return v; };
        if (o == "cand") {
            const int32_t S = (int32_t)i(), W = (int32_t)i(), mw = (int32_t)i(), band = (int32_t)i();
            printf("%d\n", colour_candidate(S, W, mw, band) ? 1 : 0);
        } else if (o == "centre") {
            const float origin = __uint_as_float((unsigned)u()), res = __uint_as_float((unsigned)u());
            printf("%u\n", __float_as_uint(colour_centre(origin, res, (int)i())));
        } else if (o == "quant") {
            printf("%u\n", colour_quant(__uint_as_float((unsigned)u())));
        } else if (o == "fold") {
            const uint32_t mw = (uint32_t)u(), n = (uint32_t)u();
            uint32_t dC[3], e[4];
            for (auto& x : dC) x = (uint32_t)u();
            for (auto& x : e) x = (uint32_t)u();
            colour_fold(mw, n, dC, e);
            printf("%u %u %u %u\n", e[0], e[1], e[2], e[3]);
        } else if (o == "voxel") {
            uint32_t e[4];
            for (auto& x : e) x = (uint32_t)u();
            const uint32_t c = colour_voxel(e);
            printf("%u %u %u %u\n", c & 255u, (c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
        } else if (o == "vertex") {
            uint32_t e[8][4];
            for (auto& r : e)
                for (auto& x : r) x = (uint32_t)u();
            const uint32_t c = colour_vertex(e);
            printf("%u %u %u %u\n", c & 255u, (c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
        } else if (o == "layer") {
            const size_t n = (size_t)u();
            std::vector<uint32_t> s(4 * n + 1);
            for (size_t k = 0; k < 4 * n; ++k) s[k] = (uint32_t)u();
            printf("%zu\n", colour_check_layer(s.data(), n));
        } else if (o == "params") {
            Ctx c;
            c.prm.view.blend = (int)i();
            c.prm.band = (int)i();
            c.prm.min_weight = (int)i();
            c.prm.max_weight = (int)i();
            g_err[0] = 0;
            const int rc = colour_rule(&c.view, 1, &c.prm, &c.q, c.cams);
            printf("%s\n", rc == LV_OK ? "ok" : g_err);
        } else {
            return 2;
        }
    }
    return 0;
}

void defaults() {
    lv_colour_params p;
    default_colour_params(&p);
    lv_paint_params v;
    default_paint_params(&v);
    CHECK(p.view.zbuf_scale == 8 && p.view.window == 1 && p.view.margin_abs == 0.5f && p.view.blend == 0);
    CHECK(p.view.min_depth == v.min_depth && p.view.max_depth == v.max_depth && p.view.max_norm_radius == v.max_norm_radius && p.view.margin_rel == v.margin_rel);
    CHECK(p.band == 256 && p.min_weight == 1 && p.max_weight == 64 && p.reserved == 0);
    default_colour_params(nullptr);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "rule") return rule();
    const std::map<std::string, void (*)()> scenarios = {{"unconfigured", unconfigured}, {"no_layer", no_layer}, {"integrate", integrate},
                                                         {"load_clear", load_clear}, {"defaults", defaults}};
    const auto it = scenarios.find(s);
    if (it == scenarios.end()) return 2;
    it->second();
    printf("ok %s\n", s.c_str());
    return 0;
}
