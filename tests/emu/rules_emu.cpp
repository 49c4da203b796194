// tests/emu/rules_emu.cpp — HOST test of the map tools' argument rules (limo-velo_amd/csrc/lv_rules.hpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_rules_host.py with AddressSanitizer + UndefinedBehaviorSanitizer, never shipped.  It
// compiles the product's own header with plain g++ (no HIP stand-in is needed) and answers one case per line of stdin:
//   <tool> key=v[,v...] ...     the fields set on the tool's defaults; ints in decimal, f32 / f64 as the decimal of their bit patterns;
//                               null_<argument>=1, n_views=N and v<i>.<field>= for the views (each a valid default view otherwise)
//   defaults <tool>             the tool's lv_default_*_params
// with one line: <rc> TAB <message> TAB <the resolved rule's fields> [TAB <one PaintCam's fields>]..., in the same number format.
// A key no tool reads is an error (exit 2): a misspelt field cannot pass for a default.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../limo-velo_amd/csrc/lv_rules.hpp"

using namespace lv;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

struct Args {
    std::map<std::string, std::vector<uint64_t>> kv;
    std::set<std::string> used;
    const std::vector<uint64_t>* find(const std::string& k, size_t n) {
        auto it = kv.find(k);
        if (it == kv.end()) return nullptr;
        if (n && it->second.size() != n) { fprintf(stderr, "%s: %zu values, %zu expected\n", k.c_str(), it->second.size(), n); std::exit(2); }
        used.insert(k);
        return &it->second;
    }
    template <class T>
    void num(const std::string& k, T* dst) { if (auto v = find(k, 1)) *dst = (T)(int64_t)(*v)[0]; }
    void f32(const std::string& k, float* dst, size_t n = 1) {
        if (auto v = find(k, n)) for (size_t i = 0; i < n; ++i) { const uint32_t b = (uint32_t)(*v)[i]; std::memcpy(dst + i, &b, 4); }
    }
    void f64(const std::string& k, double* dst, size_t n = 1) {
        if (auto v = find(k, n)) for (size_t i = 0; i < n; ++i) std::memcpy(dst + i, &(*v)[i], 8);
    }
    bool flag(const std::string& k) { int f = 0; num(k, &f); return f != 0; }
};

std::string g_out;
void put(const char* name, long long v) { g_out += std::string(g_out.empty() || g_out.back() == '\t' ? "" : " ") + name + "=" + std::to_string(v); }
void put(const char* name, unsigned long long v) { g_out += std::string(g_out.empty() || g_out.back() == '\t' ? "" : " ") + name + "=" + std::to_string(v); }
void put(const char* name, int v) { put(name, (long long)v); }
void put(const char* name, uint32_t v) { put(name, (unsigned long long)v); }
void put(const char* name, size_t v) { put(name, (unsigned long long)v); }
void put(const char* name, const float* v, size_t n = 1) {
    std::string s;
    for (size_t i = 0; i < n; ++i) { uint32_t b; std::memcpy(&b, v + i, 4); s += (i ? "," : "") + std::to_string(b); }
    g_out += std::string(g_out.empty() || g_out.back() == '\t' ? "" : " ") + name + "=" + s;
}
void put(const char* name, const double* v, size_t n = 1) {
    std::string s;
    for (size_t i = 0; i < n; ++i) { uint64_t b; std::memcpy(&b, v + i, 8); s += (i ? "," : "") + std::to_string(b); }
    g_out += std::string(g_out.empty() || g_out.back() == '\t' ? "" : " ") + name + "=" + s;
}
#define PUT(s, f) put(#f, (s).f)
#define PUTF(s, f) put(#f, &(s).f)

char g_dummy[64];   // what a valid pointer points at: the rules never read it

constexpr size_t MAX_VIEWS = 64;   // (more than any limit: the rules refuse a larger n_views before they read a view)

size_t read_views(Args& a, lv_view* views) {
    size_t n = 1;
    a.num("n_views", &n);
    for (size_t i = 0; i < MAX_VIEWS; ++i) {
        lv_view w{};
        w.R[0] = w.R[4] = w.R[8] = 1.f;
        w.stride = 12;
        const std::string pre = "v" + std::to_string(i) + ".";
        a.f32(pre + "R", w.R, 9);
        a.f32(pre + "t", w.t, 3);
        if (a.flag(pre + "points")) w.points = g_dummy;
        a.num(pre + "stride", &w.stride);
        a.num(pre + "n", &w.n);
        views[i] = w;
    }
    return n;
}

size_t read_cameras(Args& a, lv_camera_view* views) {
    size_t n = 1;
    a.num("n_views", &n);
    for (size_t i = 0; i < MAX_VIEWS; ++i) {
        lv_camera_view w{};
        w.R[0] = w.R[4] = w.R[8] = 1.f;
        w.fx = w.fy = 1.f;
        w.width = w.height = 4;
        w.format = LV_IMAGE_RGB8;
        w.row_stride = 12;
        int image = 1;
        const std::string pre = "v" + std::to_string(i) + ".";
        a.f32(pre + "R", w.R, 9);
        a.f32(pre + "t", w.t, 3);
        a.f32(pre + "fx", &w.fx);
        a.f32(pre + "fy", &w.fy);
        a.f32(pre + "cx", &w.cx);
        a.f32(pre + "cy", &w.cy);
        a.f32(pre + "dist", w.dist, 5);
        a.num(pre + "width", &w.width);
        a.num(pre + "height", &w.height);
        a.num(pre + "format", &w.format);
        a.num(pre + "image", &image);
        a.num(pre + "row_stride", &w.row_stride);
        w.image = image ? g_dummy : nullptr;
        views[i] = w;
    }
    return n;
}

void fields(Args& a, lv_visibility_params& p) {
    a.num("width", &p.width); a.num("height", &p.height); a.f32("v_min_deg", &p.v_min_deg); a.f32("v_max_deg", &p.v_max_deg);
    a.f32("min_range", &p.min_range); a.f32("max_range", &p.max_range); a.f32("margin_abs", &p.margin_abs); a.f32("margin_rel", &p.margin_rel);
    a.num("window", &p.window); a.num("min_hits", &p.min_hits); a.num("dry_run", &p.dry_run);
}
void fields(Args& a, lv_surface_params& p) {
    a.num("k", &p.k); a.f32("max_dist", &p.max_dist); a.num("min_neighbours", &p.min_neighbours); a.num("orient", &p.orient); a.f64("viewpoint", p.viewpoint, 3);
}
void fields(Args& a, lv_outlier_params& p) {
    a.num("mode", &p.mode); a.num("k", &p.k); a.f32("max_dist", &p.max_dist); a.f32("std_mul", &p.std_mul); a.f32("radius", &p.radius);
    a.num("min_neighbours", &p.min_neighbours); a.num("dry_run", &p.dry_run);
}
void fields(Args& a, lv_cluster_params& p) { a.f32("radius", &p.radius); a.num("min_size", &p.min_size); a.num("max_size", &p.max_size); a.num("dry_run", &p.dry_run); }
void fields(Args& a, lv_paint_params& p) {
    a.f32("min_depth", &p.min_depth); a.f32("max_depth", &p.max_depth); a.f32("max_norm_radius", &p.max_norm_radius); a.num("zbuf_scale", &p.zbuf_scale);
    a.num("window", &p.window); a.f32("margin_abs", &p.margin_abs); a.f32("margin_rel", &p.margin_rel); a.num("blend", &p.blend);
}
void fields(Args& a, lv_place_params& p) {
    a.num("n_rings", &p.n_rings); a.num("n_sectors", &p.n_sectors); a.f32("rmin", &p.rmin); a.f32("rmax", &p.rmax); a.f32("z_offset", &p.z_offset);
}

void show(const lv_visibility_params& p) {
    PUT(p, width); PUT(p, height); PUTF(p, v_min_deg); PUTF(p, v_max_deg); PUTF(p, min_range); PUTF(p, max_range); PUTF(p, margin_abs); PUTF(p, margin_rel);
    PUT(p, window); PUT(p, min_hits); PUT(p, dry_run);
}
void show(const lv_surface_params& p) { PUT(p, k); PUTF(p, max_dist); PUT(p, min_neighbours); PUT(p, orient); put("viewpoint", p.viewpoint, 3); }
void show(const lv_outlier_params& p) { PUT(p, mode); PUT(p, k); PUTF(p, max_dist); PUTF(p, std_mul); PUTF(p, radius); PUT(p, min_neighbours); PUT(p, dry_run); }
void show(const lv_cluster_params& p) { PUTF(p, radius); PUT(p, min_size); PUT(p, max_size); PUT(p, dry_run); }
void show(const lv_paint_params& p) {
    PUTF(p, min_depth); PUTF(p, max_depth); PUTF(p, max_norm_radius); PUT(p, zbuf_scale); PUT(p, window); PUTF(p, margin_abs); PUTF(p, margin_rel); PUT(p, blend);
}
void show(const lv_place_params& p) { PUT(p, n_rings); PUT(p, n_sectors); PUTF(p, rmin); PUTF(p, rmax); PUTF(p, z_offset); }

void show(const SurfRule& q) {
    PUT(q, job); PUT(q, k); PUT(q, min_neighbours); PUT(q, orient); PUTF(q, max_dist); PUTF(q, std_mul); put("viewpoint", q.viewpoint, 3); PUTF(q, threshold);
    PUT(q, fixed_threshold);
}

// 0xA5 in every byte: a field a lv_default_* leaves unset shows
template <class P>
P poisoned() { P p; std::memset(&p, 0xA5, sizeof(p)); return p; }

int run(const std::string& tool, Args& a) {
    if (tool == "vis") {
        lv_visibility_params p = poisoned<lv_visibility_params>();
        default_visibility_params(&p);
        fields(a, p);
        static lv_view views[MAX_VIEWS];
        const size_t n = read_views(a, views);
        VisRule q{};
        const int rc = visibility_rule(a.flag("null_views") ? nullptr : views, n, a.flag("null_params") ? nullptr : &p, &q);
        if (rc) return rc;
        PUT(q, width); PUT(q, height); PUT(q, n_views); PUT(q, window); PUT(q, min_hits); PUTF(q, inv_col); PUTF(q, v_min); PUTF(q, inv_row);
        PUTF(q, min_range); PUTF(q, max_range); PUTF(q, margin_abs); PUTF(q, margin_rel);
        return rc;
    }
    if (tool == "integrate" || tool == "gain") {   // the shared view check as lv_occ_integrate / lv_occ_view_gain call it
        static lv_view views[MAX_VIEWS];
        const size_t n = read_views(a, views);
        return views_ok(views, n, tool == "gain" ? "lv_occ_view_gain: " : "", false, 0xFFFFFFF0ull / 4);
    }
    if (tool == "normals") {
        lv_surface_params p = poisoned<lv_surface_params>();
        default_surface_params(&p);
        fields(a, p);
        SurfRule q{};
        const int rc = surface_rule(a.flag("null_params") ? nullptr : &p, &q);
        if (!rc) show(q);
        return rc;
    }
    if (tool == "outliers") {
        lv_outlier_params p = poisoned<lv_outlier_params>();
        default_outlier_params(&p);
        fields(a, p);
        SurfRule q{};
        const int rc = outlier_rule(a.flag("null_params") ? nullptr : &p, &q);
        if (!rc) show(q);
        return rc;
    }
    if (tool == "cluster") {
        lv_cluster_params p = poisoned<lv_cluster_params>();
        default_cluster_params(&p);
        fields(a, p);
        ClusterRule q{};
        const int rc = cluster_rule(a.flag("null_params") ? nullptr : &p, &q);
        if (rc) return rc;
        PUTF(q, radius); PUT(q, min_size); PUT(q, max_size); PUT(q, seeded);
        return rc;
    }
    if (tool == "paint") {
        lv_paint_params p = poisoned<lv_paint_params>();
        default_paint_params(&p);
        fields(a, p);
        static lv_camera_view views[MAX_VIEWS];
        const size_t n = read_cameras(a, views);
        PaintRule q{};
        static PaintCam cams[PAINT_MAX_VIEWS];
        std::memset(cams, 0xA5, sizeof(cams));
        const int rc = paint_rule(a.flag("null_views") ? nullptr : views, n, a.flag("null_params") ? nullptr : &p, &q, cams);
        if (rc) return rc;
        PUT(q, n_views); PUT(q, window); PUT(q, blend); PUTF(q, min_depth); PUTF(q, max_depth); PUTF(q, r2_max); PUTF(q, s); PUTF(q, margin_abs);
        PUTF(q, margin_rel); PUT(q, max_pixels); PUT(q, max_cells); PUT(q, total_pixels); PUT(q, total_cells); PUT(q, raw_bytes);
        for (size_t v = 0; v < n; ++v) {
            const PaintCam& c = cams[v];
            g_out += "\t";
            put("R", c.R, 9); put("t", c.t, 3); PUTF(c, fx); PUTF(c, fy); PUTF(c, cx); PUTF(c, cy); PUTF(c, k1); PUTF(c, k2); PUTF(c, p1); PUTF(c, p2);
            PUTF(c, k3); PUTF(c, wm1); PUTF(c, hm1); PUT(c, width); PUT(c, height); PUT(c, cw); PUT(c, ch); PUT(c, format); PUT(c, tex_off);
            PUT(c, cell_off); PUT(c, raw_off); PUT(c, pad);
        }
        return rc;
    }
    if (tool == "place_params") {
        lv_place_params p = poisoned<lv_place_params>();
        default_place_params(&p);
        fields(a, p);
        return place_params_ok(a.flag("null_params") ? nullptr : &p);
    }
    if (tool == "place_state") {
        lv_state x{};
        x.rot[3] = x.offset_R_L_I[3] = 1.0;
        a.f64("x", reinterpret_cast<double*>(&x), sizeof(lv_state) / sizeof(double));
        return place_state_ok(a.flag("null_state") ? nullptr : &x);
    }
    if (tool == "place_centres") {
        std::vector<double> cs = {1.0, 2.0, 3.0, -4.0, 5.0, 6.5};
        if (auto v = a.find("centres", 0)) {
            cs.resize(v->size());
            for (size_t i = 0; i < v->size(); ++i) std::memcpy(&cs[i], &(*v)[i], 8);
        }
        return place_centres_ok(cs.data(), cs.size() / 3);   // (exactly 3 n doubles: a read past them is ASan's to report)
    }
    if (tool == "defaults") {
        const std::string which = a.kv.empty() ? "" : a.kv.begin()->first;
        a.used.insert(which);
        // (NULL is taken and ignored)
        if (which == "vis") { default_visibility_params(nullptr); auto p = poisoned<lv_visibility_params>(); default_visibility_params(&p); show(p); }
        else if (which == "normals") { default_surface_params(nullptr); auto p = poisoned<lv_surface_params>(); default_surface_params(&p); show(p); }
        else if (which == "outliers") { default_outlier_params(nullptr); auto p = poisoned<lv_outlier_params>(); default_outlier_params(&p); show(p); }
        else if (which == "cluster") { default_cluster_params(nullptr); auto p = poisoned<lv_cluster_params>(); default_cluster_params(&p); show(p); }
        else if (which == "paint") { default_paint_params(nullptr); auto p = poisoned<lv_paint_params>(); default_paint_params(&p); show(p); }
        else if (which == "place_params") { default_place_params(nullptr); auto p = poisoned<lv_place_params>(); default_place_params(&p); show(p); }
        else { fprintf(stderr, "defaults of what: %s\n", which.c_str()); std::exit(2); }
        return LV_OK;
    }
    fprintf(stderr, "unknown tool %s\n", tool.c_str());
    std::exit(2);
}

}  // namespace

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        if (text.empty()) continue;
        std::istringstream in(text);
        std::string tool, tok;
        in >> tool;
        Args a;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            std::vector<uint64_t> vals;
            if (eq != std::string::npos) {
                std::istringstream vs(tok.substr(eq + 1));
                std::string one;
                while (std::getline(vs, one, ',')) vals.push_back(one[0] == '-' ? (uint64_t)std::strtoll(one.c_str(), nullptr, 10) : std::strtoull(one.c_str(), nullptr, 10));
            }
            a.kv[tok.substr(0, eq)] = vals;
        }
        g_out.clear();
        g_err[0] = 0;
        const int rc = run(tool, a);
        for (const auto& kv : a.kv)
            if (!a.used.count(kv.first)) { fprintf(stderr, "%s: nothing reads %s\n", tool.c_str(), kv.first.c_str()); return 2; }
        printf("%d\t%s\t%s\n", rc, g_err, g_out.c_str());
    }
    return 0;
}
