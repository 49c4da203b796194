// scripts/map_planes_host.cpp — the rule of lv_map_planes on ONE CPU core, from the library's own host-compilable header
// (limo-velo_amd/csrc/lv_planes.hpp): what scripts/map_planes_timing.py times lv_map_planes against, after lv_map_fetch has
// brought the points to the host.  Built by that script with g++ -O2 -ffp-contract=off.
//
//   map_planes_host <points.f32> <labels.i32> distance iterations max_planes min_inliers seed constraint ax ay az max_angle refine
//
// points.f32: n x 3 floats in map order.  Writes n int32 labels and prints one line: <milliseconds of the extraction> <P>
// then per plane: hypothesis support inliers n_fit.
#define LV_SURFACE_HOST_ONLY 1
#define LV_PLANES_HOST_ONLY 1
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../limo-velo_amd/csrc/lv_planes.hpp"

using namespace lv;

void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
}

int main(int argc, char** argv) {
    if (argc != 14) { fprintf(stderr, "usage: see the file header\n"); return 2; }
    lv_plane_params p;
    default_plane_params(&p);
    p.distance = strtof(argv[3], nullptr);
    p.iterations = (uint32_t)strtoul(argv[4], nullptr, 10);
    p.max_planes = (uint32_t)strtoul(argv[5], nullptr, 10);
    p.min_inliers = (uint32_t)strtoul(argv[6], nullptr, 10);
    p.seed = strtoull(argv[7], nullptr, 10);
    p.constraint = atoi(argv[8]);
    for (int a = 0; a < 3; ++a) p.axis[a] = strtof(argv[9 + a], nullptr);
    p.max_angle = strtof(argv[12], nullptr);
    p.refine = atoi(argv[13]);
    PlaneRule q;
    std::memset(&q, 0, sizeof(q));
    if (plane_rule(&p, &q)) return 2;

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t m = (size_t)ftell(f) / 12;
    fseek(f, 0, SEEK_SET);
    std::vector<float> xyz(3 * m);
    if (fread(xyz.data(), 12, m, f) != m) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);

    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> labels(m, -1);
    std::vector<uint32_t> cand;
    std::vector<float> cx, cy, cz;
    std::vector<lv_plane> planes;
    for (uint32_t r = 0; r < q.max_planes; ++r) {
        cand.clear(); cx.clear(); cy.clear(); cz.clear();
        for (size_t i = 0; i < m; ++i)
            if (labels[i] < 0) { cand.push_back((uint32_t)i); cx.push_back(xyz[3 * i]); cy.push_back(xyz[3 * i + 1]); cz.push_back(xyz[3 * i + 2]); }
        const uint32_t n = (uint32_t)cand.size();
        if (n < 3u || n < q.min_inliers) break;
        uint32_t best = 0, best_h = 0;
        float bn[3] = {0.f, 0.f, 0.f}, ba[3] = {0.f, 0.f, 0.f};
        for (uint32_t h = 0; h < q.iterations; ++h) {
            const uint32_t i0 = pl_draw(q.seed, r, h, 0, n), i1 = pl_draw(q.seed, r, h, 1, n), i2 = pl_draw(q.seed, r, h, 2, n);
            if (i0 == i1 || i0 == i2 || i1 == i2) continue;
            const float p0[3] = {cx[i0], cy[i0], cz[i0]}, p1[3] = {cx[i1], cy[i1], cz[i1]}, p2[3] = {cx[i2], cy[i2], cz[i2]};
            float nrm[3];
            if (!pl_hypothesis(p0, p1, p2, q.constraint, q.axis[0], q.axis[1], q.axis[2], q.cos_max, q.sin_max, nrm)) continue;
            uint32_t c = 0;
            for (uint32_t i = 0; i < n; ++i) c += pl_inlier(nrm[0], nrm[1], nrm[2], p0[0], p0[1], p0[2], cx[i], cy[i], cz[i], q.distance) ? 1u : 0u;
            if (c > best) { best = c; best_h = h; std::memcpy(bn, nrm, sizeof(bn)); std::memcpy(ba, p0, sizeof(ba)); }
        }
        if (best < q.min_inliers) break;
        lv_plane out;
        std::memset(&out, 0, sizeof(out));
        std::memcpy(out.normal, bn, sizeof(bn));
        std::memcpy(out.anchor, ba, sizeof(ba));
        out.support = best;
        out.hypothesis = best_h;
        out.candidates = n;
        if (q.refine) {
            long long s[PL_SUMS] = {0};
            std::vector<long long> slots;   // one per 4096 fitted points, as a workgroup of the device forms them
            uint32_t in_slot = 0;
            auto flush = [&]() { slots.insert(slots.end(), s, s + PL_SUMS); std::memset(s, 0, sizeof(s)); in_slot = 0; };
            for (uint32_t i = 0; i < n; ++i) {
                if (!pl_inlier(bn[0], bn[1], bn[2], ba[0], ba[1], ba[2], cx[i], cy[i], cz[i], q.distance)) continue;
                int32_t gx, gy, gz;
                const bool okx = pl_quant(cx[i], ba[0], &gx), oky = pl_quant(cy[i], ba[1], &gy), okz = pl_quant(cz[i], ba[2], &gz);
                if (!(okx && oky && okz)) continue;
                pl_accumulate(s, gx, gy, gz);
                if (++in_slot == 4096u) flush();
            }
            flush();
            double m6[6], s1[3];
            const uint64_t nn = pl_fold(slots.data(), slots.size() / PL_SUMS, m6, s1);
            out.n_fit = (uint32_t)nn;
            double rms = 0.0;
            if (pl_refit(nn, m6, s1, q.constraint, q.axis, out.normal, out.anchor, &rms)) out.flags |= 1u;
        }
        uint32_t members = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (pl_inlier(out.normal[0], out.normal[1], out.normal[2], out.anchor[0], out.anchor[1], out.anchor[2], cx[i], cy[i], cz[i], q.distance)) {
                labels[cand[i]] = (int32_t)r;
                ++members;
            }
        out.inliers = members;
        planes.push_back(out);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(labels.data(), 4, m, f);
    fclose(f);
    printf("%.3f %zu", ms, planes.size());
    for (const lv_plane& pl : planes) printf(" %u %u %u %u", pl.hypothesis, pl.support, pl.inliers, pl.n_fit);
    printf("\n");
    return 0;
}
