// tests/emu/tsdf_emu.cpp — the rule of limo-velo_amd/csrc/lv_tsdf.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The loops below are the loops of tsdf_march_kernel and tsdf_fold_kernel with a plain add in place
// of the atomic, then the five steps of the mesh build with running sums in place of the scans.  tests/test_tsdf_host.py holds its
// output to tests/tsdf_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   origin[3] resolution nx ny nz min_range max_range trunc_cells max_weight carve min_weight
//   n_calls, then per call: n_views, then per view: R[9] t[3] n, then n x (x y z)
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   per call: "call <used> <cut> <contributions> <touched>"
//   "S" and every voxel's S, "W" and every voxel's W, "metres" and the bits of every voxel's metres
//   "mesh <vertices> <triangles> <active> <refused>", the vertices' sub-units on one line, the bits of their metres on the next,
//   the triangles' indices on the third
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lv_tsdf.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

static float read_f() {
    unsigned int u = 0;
    if (scanf("%u", &u) != 1) exit(2);
    return __uint_as_float(u);
}
static long read_i() {
    long v = 0;
    if (scanf("%ld", &v) != 1) exit(2);
    return v;
}

int main() {
    lv_tsdf_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = read_f();
    p.resolution = read_f();
    p.nx = (int)read_i(); p.ny = (int)read_i(); p.nz = (int)read_i();
    p.min_range = read_f(); p.max_range = read_f();
    p.trunc_cells = (int)read_i(); p.max_weight = (int)read_i(); p.carve = (int)read_i();
    const int min_weight = (int)read_i();
    if (const char* why = tsdf_check_params(&p)) {
        printf("params bad: %s\n", why);
        return 0;
    }
    printf("params ok\n");
    const TsdfGrid g = tsdf_grid_of(p);
    const size_t nv = (size_t)p.nx * p.ny * p.nz;
    std::vector<int32_t> S(nv, 0), W(nv, 0);
    std::vector<unsigned long long> scratch(nv, 0);
    const long n_calls = read_i();
    for (long call = 0; call < n_calls; ++call) {
        const long n_views = read_i();
        unsigned long long used = 0, cut = 0, contributions = 0, touched = 0;
        for (long v = 0; v < n_views; ++v) {
            float R[9], t[3];
            for (float& x : R) x = read_f();
            for (float& x : t) x = read_f();
            const long n = read_i();
            std::vector<float> pts((size_t)n * 3);
            for (float& x : pts) x = read_f();
            int32_t qs[3];
            if (!(n && occ_view_origin(g.occ, t, qs))) continue;
            for (long i = 0; i < n; ++i) {
                int32_t qe[3] = {0, 0, 0};
                const int kind = occ_return(g.occ, R, t, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], qe);
                if (kind == OCC_RAY_IGNORED) continue;
                TsdfRay ray;
                if (!tsdf_ray_init(g, qs, qe, kind, ray)) continue;
                ++used;
                cut += kind == OCC_RAY_CUT;
                OccWalk w;
                occ_walk_init(w, ray.start, ray.qb);
                bool left = false;
                for (;;) {
                    if (occ_in_grid(g.occ, w.vx, w.vy, w.vz)) {
                        int32_t s;
                        if (tsdf_cell_s(g, ray, w.vx, w.vy, w.vz, s)) {
                            if (s < -g.T || s > g.T) { printf("s out of the band\n"); return 3; }
                            scratch[grid_at(g.occ, w.vx, w.vy, w.vz)] += tsdf_pack(s);
                        }
                    } else if (occ_walk_left(g.occ, w)) {
                        left = true;
                        break;
                    }
                    if (occ_walk_done(w)) break;
                    occ_walk_step(w);
                }
                if (!left && (w.vx != w.ex || w.vy != w.ey || w.vz != w.ez)) { printf("walk did not end in ve\n"); return 3; }
            }
        }
        for (size_t i = 0; i < nv; ++i) {
            if (!scratch[i]) continue;
            int64_t dS, dW;
            tsdf_unpack(scratch[i], dS, dW);
            if (dW <= 0) { printf("a word without weight\n"); return 3; }
            tsdf_fold(g.max_weight, dS, dW, S[i], W[i]);
            scratch[i] = 0;
            contributions += (unsigned long long)dW;
            ++touched;
        }
        printf("call %llu %llu %llu %llu\n", used, cut, contributions, touched);
    }
    printf("S\n");
    for (size_t i = 0; i < nv; ++i) printf("%d ", S[i]);
    printf("\nW\n");
    for (size_t i = 0; i < nv; ++i) printf("%d ", W[i]);
    printf("\nmetres\n");
    for (size_t i = 0; i < nv; ++i) printf("%u ", __float_as_uint(tsdf_metres(p.resolution, S[i], W[i])));
    printf("\n");
    if (tsdf_check_volume(g, S.data(), W.data(), nv) != nv) { printf("the volume breaks |S| <= T * W\n"); return 3; }

    // the mesh: classify, number, vertices, count faces, emit
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
            sub[3 * vid[cell] + a] = v[a];
            xyz[3 * vid[cell] + a] = tsdf_vertex_metres(p.origin[a], p.resolution, v[a]);
        }
    }
    std::vector<uint32_t> tri;
    unsigned long long refused = 0;
    const uint32_t* fl = flag.data();
    for (size_t cell = 0; cell < nv; ++cell) {
        int i, j, k;
        grid_ijk(d, (uint32_t)cell, i, j, k);
        uint32_t q[4];
        for (int a = 0; a < 3; ++a) {
            const int r = tsdf_edge_face(d, S.data(), W.data(), min_weight, i, j, k, a, [fl](uint32_t c) { return fl[c] != 0; }, q);
            refused += r == 2;
            if (r != 1) continue;
            const uint32_t v[4] = {vid[q[0]], vid[q[1]], vid[q[2]], vid[q[3]]};
            const uint32_t six[6] = {v[0], v[1], v[2], v[0], v[2], v[3]};
            tri.insert(tri.end(), six, six + 6);
        }
    }
    printf("mesh %u %zu %u %llu\n", n_vert, tri.size() / 3, n_vert, refused);
    for (int32_t v : sub) printf("%d ", v);
    printf("\n");
    for (float v : xyz) printf("%u ", __float_as_uint(v));
    printf("\n");
    for (uint32_t v : tri) printf("%u ", v);
    printf("\n");
    return 0;
}
