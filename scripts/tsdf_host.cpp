// scripts/tsdf_host.cpp — the host side of scripts/tsdf_timing.py: the rule of limo-velo_amd/csrc/lv_tsdf.hpp (what
// tests/emu/tsdf_emu.cpp runs) built with g++ -O2 through tests/emu/hip/hip_runtime.h, on binary files, timing itself: what a
// caller pays who fuses the sweeps and extracts the mesh on one CPU core.
//
//   tsdf_host PARAMS VIEWS
// PARAMS: origin[3] resolution min_range max_range (f32), then nx ny nz trunc_cells max_weight carve min_weight (i32).
// VIEWS: i32 n_views; then per view R[9] t[3] f32 and i32 n; then every view's n x 3 f32 returns, view after view.
// stdout: one JSON object: integrate_ms (all views as one call, the fold included), the call's four stats, mesh_ms, vertices,
// triangles, refused.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lv_tsdf.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

static std::vector<char> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> v((size_t)bytes);
    if (fread(v.data(), 1, v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::vector<char> pb = slurp(argv[1]);
    if (pb.size() != 6 * sizeof(float) + 7 * sizeof(int32_t)) return 2;
    float pf[6];
    int32_t pi[7];
    std::memcpy(pf, pb.data(), sizeof(pf));
    std::memcpy(pi, pb.data() + sizeof(pf), sizeof(pi));
    lv_tsdf_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = pf[a];
    p.resolution = pf[3]; p.min_range = pf[4]; p.max_range = pf[5];
    p.nx = pi[0]; p.ny = pi[1]; p.nz = pi[2]; p.trunc_cells = pi[3]; p.max_weight = pi[4]; p.carve = pi[5];
    const int min_weight = pi[6];
    if (const char* why = tsdf_check_params(&p)) { fprintf(stderr, "%s\n", why); return 2; }
    const TsdfGrid g = tsdf_grid_of(p);
    const size_t nv = grid_cells(g.occ);

    const std::vector<char> vb = slurp(argv[2]);
    int32_t n_views = 0;
    std::memcpy(&n_views, vb.data(), sizeof(n_views));
    const char* head = vb.data() + sizeof(int32_t);
    const size_t rec = 12 * sizeof(float) + sizeof(int32_t);
    const float* pts = reinterpret_cast<const float*>(head + rec * (size_t)n_views);   // (4-byte aligned: every field before it is 4 bytes)

    std::vector<int32_t> S(nv, 0), W(nv, 0);
    std::vector<unsigned long long> scratch(nv, 0);
    unsigned long long used = 0, cut = 0, contributions = 0, touched = 0;
    auto t0 = std::chrono::steady_clock::now();
    for (int v = 0; v < n_views; ++v) {
        float pose[12];
        int32_t n = 0;
        std::memcpy(pose, head + rec * (size_t)v, sizeof(pose));
        std::memcpy(&n, head + rec * (size_t)v + sizeof(pose), sizeof(n));
        const float* R = pose;
        const float* t = pose + 9;
        int32_t qs[3];
        if (n && occ_view_origin(g.occ, t, qs)) {
            for (int32_t i = 0; i < n; ++i) {
                int32_t qe[3] = {0, 0, 0};
                const int kind = occ_return(g.occ, R, t, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], qe);
                if (kind == OCC_RAY_IGNORED) continue;
                TsdfRay ray;
                if (!tsdf_ray_init(g, qs, qe, kind, ray)) continue;
                ++used;
                cut += kind == OCC_RAY_CUT;
                OccWalk w;
                occ_walk_init(w, ray.start, ray.qb);
                for (;;) {
                    if (occ_in_grid(g.occ, w.vx, w.vy, w.vz)) {
                        int32_t s;
                        if (tsdf_cell_s(g, ray, w.vx, w.vy, w.vz, s)) scratch[grid_at(g.occ, w.vx, w.vy, w.vz)] += tsdf_pack(s);
                    } else if (occ_walk_left(g.occ, w)) {
                        break;
                    }
                    if (occ_walk_done(w)) break;
                    occ_walk_step(w);
                }
            }
        }
        pts += 3 * (size_t)n;
    }
    for (size_t i = 0; i < nv; ++i) {
        if (!scratch[i]) continue;
        int64_t dS, dW;
        tsdf_unpack(scratch[i], dS, dW);
        tsdf_fold(g.max_weight, dS, dW, S[i], W[i]);
        scratch[i] = 0;
        contributions += (unsigned long long)dW;
        ++touched;
    }
    const double integrate_ms = ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    const GridDims d{p.nx, p.ny, p.nz};
    std::vector<uint32_t> flag(nv, 0), vid(nv, 0);
    uint32_t n_vert = 0;
    for (size_t cell = 0; cell < nv; ++cell) {
        int i, j, k;
        grid_ijk(d, (uint32_t)cell, i, j, k);
        TsdfCorners c;
        flag[cell] = tsdf_cell_active(d, S.data(), W.data(), min_weight, i, j, k, c) ? 1u : 0u;
        vid[cell] = n_vert;
        n_vert += flag[cell];
    }
    std::vector<int32_t> sub(3 * (size_t)n_vert);
    std::vector<float> xyz(3 * (size_t)n_vert);
    for (size_t cell = 0; cell < nv; ++cell) {
        if (!flag[cell]) continue;
        int i, j, k;
        grid_ijk(d, (uint32_t)cell, i, j, k);
        TsdfCorners c;
        tsdf_cell_active(d, S.data(), W.data(), min_weight, i, j, k, c);
        int32_t v[3];
        tsdf_vertex(c, i, j, k, v);
        for (int a = 0; a < 3; ++a) {
            sub[3 * (size_t)vid[cell] + a] = v[a];
            xyz[3 * (size_t)vid[cell] + a] = tsdf_vertex_metres(p.origin[a], p.resolution, v[a]);
        }
    }
    std::vector<uint32_t> tri;
    unsigned long long refused = 0;
    const uint32_t* fl = flag.data();
    for (size_t cell = 0; cell < nv; ++cell) {
        if (W[cell] < min_weight) continue;   // (no edge starts at a voxel that is not known)
        int i, j, k;
        grid_ijk(d, (uint32_t)cell, i, j, k);
        uint32_t q[4];
        for (int a = 0; a < 3; ++a) {
            const int r = tsdf_edge_face(d, S.data(), W.data(), min_weight, i, j, k, a, [fl](uint32_t c) { return fl[c] != 0; }, q);
            refused += r == 2;
            if (r != 1) continue;
            const uint32_t six[6] = {vid[q[0]], vid[q[1]], vid[q[2]], vid[q[0]], vid[q[2]], vid[q[3]]};
            tri.insert(tri.end(), six, six + 6);
        }
    }
    const double mesh_ms = ms_since(t0);
    printf("{\"integrate_ms\": %.3f, \"stats\": [%llu, %llu, %llu, %llu], \"mesh_ms\": %.3f, \"vertices\": %u, \"triangles\": %zu, "
           "\"refused\": %llu}\n", integrate_ms, used, cut, contributions, touched, mesh_ms, n_vert, tri.size() / 3, refused);
    return 0;
}
