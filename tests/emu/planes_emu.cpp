// tests/emu/planes_emu.cpp — HOST test of the plain arithmetic of lv_map_planes (limo-velo_amd/csrc/lv_planes.hpp, with sym3_eig and
// surf_sign of lv_surface.hpp).  TEST INFRASTRUCTURE ONLY: built by tests/test_planes_host.py with plain g++, AddressSanitizer +
// UndefinedBehaviorSanitizer, never shipped.  It answers one request per line of stdin with one line of stdout; integers in
// decimal, f32 / f64 as the decimal of their bit patterns:
//   draw seed r h j n                                  -> index
//   hyp p0[3] p1[3] p2[3] constraint axis[3] cos sin   -> valid normal[3]          (f32 points, f64 axis and thresholds)
//   test normal[3] anchor[3] p[3] distance             -> s inlier
//   quant p a                                          -> ok g
//   fold n_slots slot[10 n_slots]                      -> n_fit m[6] s1[3]         (int64 slots, signed decimal)
//   refit n_fit m[6] s1[3] constraint axis[3] normal[3] anchor[3] -> done normal[3] anchor[3] rms d
//   eig c[6]                                           -> l[3] v0[3]
//   rule key=v[,v,v] ...                               -> rc TAB message TAB the resolved rule's fields   (null=1: a NULL params)
//   defaults                                           -> the fields of lv_default_plane_params
//   geometry                                           -> PL_CHUNK PL_TILE PL_FIT_PER
// A key the rule does not read is an error (exit 2).
#define LV_SURFACE_HOST_ONLY 1
#define LV_PLANES_HOST_ONLY 1
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../limo-velo_amd/csrc/lv_planes.hpp"

using namespace lv;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

struct In {
    std::istringstream s;
    explicit In(const std::string& line) : s(line) {}
    uint64_t u() {
        std::string t;
        if (!(s >> t)) { fprintf(stderr, "missing value\n"); std::exit(2); }
        return t[0] == '-' ? (uint64_t)std::strtoll(t.c_str(), nullptr, 10) : std::strtoull(t.c_str(), nullptr, 10);
    }
    float f() { const uint32_t b = (uint32_t)u(); float v; std::memcpy(&v, &b, 4); return v; }
    double d() { const uint64_t b = u(); double v; std::memcpy(&v, &b, 8); return v; }
    void f3(float* v) { for (int i = 0; i < 3; ++i) v[i] = f(); }
    void d3(double* v) { for (int i = 0; i < 3; ++i) v[i] = d(); }
};

std::string bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return std::to_string(b); }
std::string bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return std::to_string(b); }

std::string params_fields(const lv_plane_params& p) {
    std::string o;
    o += "distance=" + bits(p.distance) + " iterations=" + std::to_string(p.iterations) + " max_planes=" + std::to_string(p.max_planes);
    o += " min_inliers=" + std::to_string(p.min_inliers) + " seed=" + std::to_string(p.seed) + " constraint=" + std::to_string(p.constraint);
    o += " axis=" + bits(p.axis[0]) + "," + bits(p.axis[1]) + "," + bits(p.axis[2]) + " max_angle=" + bits(p.max_angle);
    o += " refine=" + std::to_string(p.refine);
    return o;
}

std::vector<uint64_t> values(const std::string& v) {
    std::vector<uint64_t> out;
    std::istringstream s(v);
    std::string t;
    while (std::getline(s, t, ',')) out.push_back(t[0] == '-' ? (uint64_t)std::strtoll(t.c_str(), nullptr, 10) : std::strtoull(t.c_str(), nullptr, 10));
    return out;
}

void need(const std::string& k, const std::vector<uint64_t>& v, size_t n) {
    if (v.size() != n) { fprintf(stderr, "%s: %zu values, %zu expected\n", k.c_str(), v.size(), n); std::exit(2); }
}

void do_rule(In& in) {
    lv_plane_params p;
    default_plane_params(&p);
    bool null = false;
    std::string tok;
    while (in.s >> tok) {
        const size_t eq = tok.find('=');
        const std::string k = tok.substr(0, eq);
        const std::vector<uint64_t> v = values(tok.substr(eq + 1));
        auto f32 = [&](float* dst, size_t n) { need(k, v, n); for (size_t i = 0; i < n; ++i) { const uint32_t b = (uint32_t)v[i]; std::memcpy(dst + i, &b, 4); } };
        if (k == "null") { need(k, v, 1); null = v[0] != 0; }
        else if (k == "distance") f32(&p.distance, 1);
        else if (k == "iterations") { need(k, v, 1); p.iterations = (uint32_t)v[0]; }
        else if (k == "max_planes") { need(k, v, 1); p.max_planes = (uint32_t)v[0]; }
        else if (k == "min_inliers") { need(k, v, 1); p.min_inliers = (uint32_t)v[0]; }
        else if (k == "seed") { need(k, v, 1); p.seed = v[0]; }
        else if (k == "constraint") { need(k, v, 1); p.constraint = (int)(int64_t)v[0]; }
        else if (k == "axis") f32(p.axis, 3);
        else if (k == "max_angle") f32(&p.max_angle, 1);
        else if (k == "refine") { need(k, v, 1); p.refine = (int)(int64_t)v[0]; }
        else { fprintf(stderr, "nothing reads %s\n", k.c_str()); std::exit(2); }
    }
    PlaneRule q;
    std::memset(&q, 0, sizeof(q));
    g_err[0] = 0;
    const int rc = plane_rule(null ? nullptr : &p, &q);
    std::string o = std::to_string(rc) + "\t" + g_err + "\t";
    o += "distance=" + bits(q.distance) + " iterations=" + std::to_string(q.iterations) + " max_planes=" + std::to_string(q.max_planes);
    o += " min_inliers=" + std::to_string(q.min_inliers) + " seed=" + std::to_string(q.seed) + " constraint=" + std::to_string(q.constraint);
    o += " refine=" + std::to_string(q.refine) + " axis=" + bits(q.axis[0]) + "," + bits(q.axis[1]) + "," + bits(q.axis[2]);
    o += " cos_max=" + bits(q.cos_max) + " sin_max=" + bits(q.sin_max);
    puts(o.c_str());
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        In in(line);
        std::string cmd;
        in.s >> cmd;
        if (cmd == "draw") {
            const uint64_t seed = in.u();
            const uint32_t r = (uint32_t)in.u(), h = (uint32_t)in.u(), j = (uint32_t)in.u(), n = (uint32_t)in.u();
            printf("%u\n", pl_draw(seed, r, h, j, n));
        } else if (cmd == "hyp") {
            float p0[3], p1[3], p2[3], nrm[3];
            double ax[3];
            in.f3(p0); in.f3(p1); in.f3(p2);
            const int constraint = (int)in.u();
            in.d3(ax);
            const double cm = in.d(), sm = in.d();
            const bool ok = pl_hypothesis(p0, p1, p2, constraint, ax[0], ax[1], ax[2], cm, sm, nrm);
            printf("%d %s %s %s\n", ok ? 1 : 0, bits(nrm[0]).c_str(), bits(nrm[1]).c_str(), bits(nrm[2]).c_str());
        } else if (cmd == "test") {
            float n[3], a[3], p[3];
            in.f3(n); in.f3(a); in.f3(p);
            const float dist = in.f();
            printf("%s %d\n", bits(pl_signed(n[0], n[1], n[2], a[0], a[1], a[2], p[0], p[1], p[2])).c_str(),
                   pl_inlier(n[0], n[1], n[2], a[0], a[1], a[2], p[0], p[1], p[2], dist) ? 1 : 0);
        } else if (cmd == "quant") {
            const float p = in.f(), a = in.f();
            int32_t g = 0;
            const bool ok = pl_quant(p, a, &g);
            printf("%d %d\n", ok ? 1 : 0, g);
        } else if (cmd == "fold") {
            const size_t ns = (size_t)in.u();
            std::vector<long long> slots(ns * PL_SUMS);
            for (auto& v : slots) v = (long long)in.u();
            double m[6], s1[3];
            const uint64_t n_fit = pl_fold(slots.data(), ns, m, s1);
            std::string o = std::to_string(n_fit);
            for (double v : m) o += " " + bits(v);
            for (double v : s1) o += " " + bits(v);
            puts(o.c_str());
        } else if (cmd == "refit") {
            const uint64_t n_fit = in.u();
            double m[6], s1[3], ax[3], rms = NAN;
            float nrm[3], anc[3];
            for (double& v : m) v = in.d();
            in.d3(s1);
            const int constraint = (int)in.u();
            in.d3(ax);
            in.f3(nrm); in.f3(anc);
            const bool done = pl_refit(n_fit, m, s1, constraint, ax, nrm, anc, &rms);
            std::string o = std::to_string(done ? 1 : 0);
            for (float v : nrm) o += " " + bits(v);
            for (float v : anc) o += " " + bits(v);
            o += " " + bits(rms) + " " + bits(pl_offset(nrm, anc));
            puts(o.c_str());
        } else if (cmd == "eig") {
            double c[6], l[3], v[3];
            for (double& x : c) x = in.d();
            sym3_eig(c, l, v);
            std::string o;
            for (double x : l) o += bits(x) + " ";
            for (double x : v) o += bits(x) + " ";
            o.pop_back();
            puts(o.c_str());
        } else if (cmd == "rule") {
            do_rule(in);
        } else if (cmd == "defaults") {
            lv_plane_params p;
            std::memset(&p, 0xAB, sizeof(p));
            default_plane_params(&p);
            puts(params_fields(p).c_str());
        } else if (cmd == "geometry") {
            printf("%d %d %d\n", PL_CHUNK, PL_TILE, PL_FIT_PER);
        } else {
            fprintf(stderr, "unknown request %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
