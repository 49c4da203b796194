// tests/emu/surf_merge_emu.cpp — HOST test of the submap merge's rule (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h; built and run by tests/test_surf_merge_host.py, never shipped).  It compiles the product's own
// limo-velo_amd/csrc/lv_surf_merge.hpp, unchanged.  Floats travel as their bits (f32 as uint32, f64 as uint64).
//   surf_merge_emu merge    one call read from stdin, numbers separated by white space:
//                             dest: origin[3] res nx ny nz trunc_cells max_weight
//                             sub:  origin[3] res nx ny nz trunc_cells
//                             pose: t[3] q[4] (f64 bits), then min_weight interp
//                             the submap's S then W, the destination's S then W (x fastest)
//                           It goes through surf_merge_rule, surf_merge_scale and surf_merge_box and then walks the box tile by tile
//                           as the kernel of lv_surf_merge.hip does: a tile that surf_merge_tile_outside gives up is not judged.
//                           Answer: "rc <rc> kq <kq>", "box <any> lo[3] hi[3]", "stats s[4]", then one line per destination voxel:
//                             judged state dS dW e[3] S W     (judged 0: outside the box or in a tile given up; state, dS, dW, e
//                             are then those of the full rule on that voxel all the same, S and W are the volume after the call)
//   surf_merge_emu rule     per line of stdin "<what> <value>": surf_merge_rule (and surf_merge_scale) on a good call with one
//                           thing changed -> "ok <kq>" or the refusal's message
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../../limo-velo_amd/csrc/lv_surf_merge.hpp"

using namespace lv;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

float f32_in() {
    uint32_t b;
    std::cin >> b;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
double f64_in() {
    uint64_t b;
    std::cin >> b;
    double f;
    std::memcpy(&f, &b, 8);
    return f;
}
void volume_in(std::vector<int32_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i) std::cin >> v[i];
}

int merge() {
    lv_tsdf_params dp;
    default_tsdf_params(&dp);
    for (int a = 0; a < 3; ++a) dp.origin[a] = f32_in();
    dp.resolution = f32_in();
    std::cin >> dp.nx >> dp.ny >> dp.nz >> dp.trunc_cells >> dp.max_weight;
    lv_surf_submap sub{};
    for (int a = 0; a < 3; ++a) sub.origin[a] = f32_in();
    sub.resolution = f32_in();
    std::cin >> sub.nx >> sub.ny >> sub.nz >> sub.trunc_cells;
    lv_graph_pose pose{};
    for (int a = 0; a < 3; ++a) pose.t[a] = f64_in();
    for (int a = 0; a < 4; ++a) pose.q[a] = f64_in();
    lv_surf_merge_params prm;
    default_surf_merge_params(&prm);
    std::cin >> prm.min_weight >> prm.interp;
    std::vector<int32_t> sS, sW, S, W;
    const size_t ns = (size_t)sub.nx * sub.ny * sub.nz, nd = (size_t)dp.nx * dp.ny * dp.nz;
    volume_in(sS, ns);
    volume_in(sW, ns);
    volume_in(S, nd);
    volume_in(W, nd);
    if (!std::cin) { fprintf(stderr, "short input\n"); return 2; }
    sub.S = sS.data();
    sub.W = sW.data();
    const TsdfGrid g = tsdf_grid_of(dp);
    SurfMergeRule q;
    int rc = surf_merge_rule(&sub, &pose, &prm, &q);
    if (!rc) rc = surf_merge_scale(sub.resolution, dp.resolution, &q.kq);
    printf("rc %d kq %lld\n", rc, rc ? 0ll : (long long)q.kq);
    if (rc) { printf("%s\n", g_err); return 0; }
    std::vector<MergePair> sw(ns);
    surf_merge_stage(sub, sw.data());
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    const bool any = surf_merge_box(g, q, lo, hi);
    printf("box %d %d %d %d %d %d %d\n", any ? 1 : 0, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    std::vector<uint8_t> judged(nd, 0);
    uint64_t stats[4] = {0, 0, 0, 0};
    const float res = g.occ.resolution;
    const float* o = g.occ.origin;
    if (any)
        for (int k0 = lo[2]; k0 < hi[2]; k0 += MERGE_TILE_Z)
            for (int j0 = lo[1]; j0 < hi[1]; j0 += MERGE_TILE_Y)
                for (int i0 = lo[0]; i0 < hi[0]; i0 += MERGE_TILE_X) {
                    const int i1 = std::min(i0 + MERGE_TILE_X, hi[0]) - 1, j1 = std::min(j0 + MERGE_TILE_Y, hi[1]) - 1, k1 = std::min(k0 + MERGE_TILE_Z, hi[2]) - 1;
                    const float tlo[3] = {colour_centre(o[0], res, i0), colour_centre(o[1], res, j0), colour_centre(o[2], res, k0)};
                    const float thi[3] = {colour_centre(o[0], res, i1), colour_centre(o[1], res, j1), colour_centre(o[2], res, k1)};
                    if (surf_merge_tile_outside(q, tlo, thi)) continue;
                    for (int k = k0; k <= k1; ++k)
                        for (int j = j0; j <= j1; ++j)
                            for (int i = i0; i <= i1; ++i) {
                                const float p[3] = {colour_centre(o[0], res, i), colour_centre(o[1], res, j), colour_centre(o[2], res, k)};
                                int64_t dS, dW;
                                const int st = surf_merge_voxel(q, g.T, p, sw.data(), dS, dW);
                                const size_t at = grid_at(g.occ, i, j, k);
                                judged[at] = 1;
                                stats[0] += st != MERGE_OUTSIDE;
                                stats[3] += st == MERGE_KNOWN && dW == 0;
                                if (dW > 0) {
                                    tsdf_fold(g.max_weight, dS, dW, S[at], W[at]);
                                    stats[1] += 1;
                                    stats[2] += (uint64_t)dW;
                                }
                            }
                }
    printf("stats %llu %llu %llu %llu\n", (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2], (unsigned long long)stats[3]);
    for (int k = 0; k < dp.nz; ++k)
        for (int j = 0; j < dp.ny; ++j)
            for (int i = 0; i < dp.nx; ++i) {
                const float p[3] = {colour_centre(o[0], res, i), colour_centre(o[1], res, j), colour_centre(o[2], res, k)};
                int64_t dS, dW, e[3] = {0, 0, 0};
                const int st = surf_merge_voxel(q, g.T, p, sw.data(), dS, dW);
                if (!surf_merge_lattice(q, p, e)) e[0] = e[1] = e[2] = 0;
                const size_t at = grid_at(g.occ, i, j, k);
                printf("%d %d %lld %lld %lld %lld %lld %d %d\n", (int)judged[at], st, (long long)dS, (long long)dW, (long long)e[0], (long long)e[1], (long long)e[2],
                       S[at], W[at]);
            }
    return 0;
}

// a good call with one thing changed
int rule() {
    std::string what, value;
    while (std::cin >> what >> value) {
        const double v = value == "nan" ? std::numeric_limits<double>::quiet_NaN() : value == "inf" ? std::numeric_limits<double>::infinity() : std::stod(value);
        std::vector<int32_t> S(4 * 3 * 2, 0), W(4 * 3 * 2, 1);
        lv_surf_submap sub{};
        sub.resolution = 0.2f;
        sub.nx = 4; sub.ny = 3; sub.nz = 2;
        sub.trunc_cells = 3;
        sub.S = S.data();
        sub.W = W.data();
        lv_graph_pose pose{};
        pose.q[3] = 1.0;
        lv_surf_merge_params prm;
        default_surf_merge_params(&prm);
        const lv_surf_submap* subp = &sub;
        const lv_graph_pose* posep = &pose;
        const lv_surf_merge_params* prmp = &prm;
        float dest_res = 0.2f;
        if (what == "ok") {}
        else if (what == "sub") subp = nullptr;
        else if (what == "pose") posep = nullptr;
        else if (what == "params") prmp = nullptr;   // (the defaults)
        else if (what == "origin") sub.origin[1] = (float)v;
        else if (what == "resolution") sub.resolution = (float)v;
        else if (what == "nx") sub.nx = (int)v;
        else if (what == "ny") sub.ny = (int)v;
        else if (what == "nz") sub.nz = (int)v;
        else if (what == "voxels") { sub.nx = 1024; sub.ny = 1024; sub.nz = (int)v; }   // (only refusals: the arrays are not that long)
        else if (what == "trunc_cells") sub.trunc_cells = (int)v;
        else if (what == "S") sub.S = nullptr;
        else if (what == "W") sub.W = nullptr;
        else if (what == "t") pose.t[2] = v;
        else if (what == "q") pose.q[0] = v;
        else if (what == "qnorm") pose.q[3] = v;
        else if (what == "min_weight") prm.min_weight = (int)v;
        else if (what == "interp") prm.interp = (int)v;
        else if (what == "w5") W[5] = (int)v;
        else if (what == "s7") S[7] = (int)v;
        else if (what == "dest_resolution") dest_res = (float)v;
        else { fprintf(stderr, "unknown field %s\n", what.c_str()); return 2; }
        g_err[0] = 0;
        SurfMergeRule q;
        int rc = surf_merge_rule(subp, posep, prmp, &q);
        if (!rc) rc = surf_merge_scale(sub.resolution, dest_res, &q.kq);
        if (rc) printf("%s\n", g_err);
        else printf("ok %lld %d %d\n", (long long)q.kq, q.min_weight, q.interp);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: surf_merge_emu merge | rule\n"); return 2; }
    const std::string s = argv[1];
    if (s == "merge") return merge();
    if (s == "rule") return rule();
    fprintf(stderr, "unknown mode %s\n", s.c_str());
    return 2;
}
