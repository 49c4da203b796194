// lv_graph.hip — pose-graph optimisation (include/limovelo_hip.h "Pose graph"): the kernels that run the rule of lv_graph.hpp and
// the Levenberg-Marquardt loop that drives them.
//
// Plain stream launches, no captured graphs, no grid-wide barriers or spins, no float atomics.  Every sum has one order:
//   graph_linearise_kernel   one lane per factor (edges, then priors): r, s, w, rho and, in full mode, the weighted blocks (Ji^T W Jj
//                            once per edge); the workgroup's sum of rho goes to its partial;
//   graph_gather_kernel      one lane per node: the diagonal block and the gradient summed over the node's incidence list in list
//                            order; graph_gather_long_kernel gives a node whose list is longer than 64 entries a wavefront (lane l
//                            takes entries l, l + 64, ... in order, then an xor-butterfly: a + b == b + a, so all lanes agree);
//   graph_precond_kernel     per node the inverse of the block of H + lambda diag H (graph_block_inverse);
//   pcg_*                    one conjugate-gradient iteration is three launches: the block-row product A p by the same walk of the
//                            lists with the workgroup partials of p^T A p (pcg_spmv); d, r, z updated with the partials of r^T z
//                            (pcg_update); p updated (pcg_direction).  A dot product is folded a second time by EVERY workgroup
//                            of the launch that needs it, in the same fixed order, so all of them hold the same bits and no
//                            launch of one workgroup stands between.  alpha, beta and the stop test never leave the device
//                            (GraphScalars); iterations are enqueued GRAPH_PCG_CHUNK at a time, and once the stop flag is up
//                            the launches left in the chunk return at their first instruction;
//   graph_retract_kernel     one lane per node: the trial pose and the partial of the step's max-norm;
//   graph_fold_kernel        one workgroup: the second stage of the cost and of the step norm.
// A small graph is launch-bound in this form (DESIGN.md "Pose graph" has the measurements asked for and what is still open).
#include "lv_graph.hpp"

#include <algorithm>
#include <vector>

namespace lv {

namespace {

constexpr int GB = 256;   // lanes per workgroup of every kernel here

struct GraphView {
    uint32_t n, n_edges, n_priors;
    const uint8_t* fixed;
    const uint32_t* ij;
    const uint32_t* start;
    const uint32_t* items;
    const double* elin;
    const double* plin;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}
// the workgroup's sum (or maximum), the same bits in every lane: wavefronts by butterfly, then the four of them in order
template <bool MAX>
__device__ __forceinline__ double block_fold(double v, double* sh) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();   // (sh may still be read from the previous fold)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int w = 1; w < GB / 64; ++w) t = MAX ? (sh[w] > t ? sh[w] : t) : t + sh[w];
    return t;
}
// the second stage: lane t takes partials t, t + 256, ... in order, then the workgroup's fold
template <bool MAX>
__device__ __forceinline__ double fold_partials(const double* part, uint32_t nb, double* sh) {
    double a = 0.0;
    for (uint32_t k = threadIdx.x; k < nb; k += GB) a = MAX ? (part[k] > a ? part[k] : a) : a + part[k];
    return block_fold<MAX>(a, sh);
}

__global__ __launch_bounds__(GB) void graph_linearise_kernel(const lv_graph_pose* __restrict__ x, const lv_graph_edge* __restrict__ edges,
                                                             uint32_t n_edges, const lv_graph_prior* __restrict__ priors, uint32_t n_priors,
                                                             double* __restrict__ elin, double* __restrict__ plin, double* __restrict__ s_out,
                                                             double* __restrict__ part, int full) {
    __shared__ double sh[GB / 64];
    const uint32_t f = blockIdx.x * GB + threadIdx.x;
    double rho = 0.0;
    if (f < n_edges) {
        const lv_graph_edge& e = edges[f];
        double r[6], s, w;
        rho = graph_edge_linearise(x[e.i], x[e.j], e, r, &s, &w, full ? elin + (size_t)f * GRAPH_EDGE_LIN : nullptr);
        s_out[f] = s;
    } else if (f < n_edges + n_priors) {
        const uint32_t k = f - n_edges;
        const lv_graph_prior& p = priors[k];
        double r[6], s, w;
        rho = graph_prior_linearise(x[p.i], p, r, &s, &w, full ? plin + (size_t)k * GRAPH_PRIOR_LIN : nullptr);
        s_out[f] = s;
    }
    const double t = block_fold<false>(rho, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// acc (42: block, gradient) += the entries off, off + stride, ... of the node's list
__device__ __forceinline__ void diag_terms(const GraphView& g, uint32_t node, uint32_t off, uint32_t stride, double* acc) {
    const uint32_t b = g.start[node], e = g.start[node + 1];
    for (uint32_t k = b + off; k < e; k += stride) {
        const uint32_t it = g.items[k], id = it >> 2, kind = it & 3u;
        const double* H;
        const double* gg;
        if (kind == GRAPH_PRIOR) {
            H = g.plin + (size_t)id * GRAPH_PRIOR_LIN;
            gg = H + 36;
        } else {
            const double* base = g.elin + (size_t)id * GRAPH_EDGE_LIN;
            H = base + (kind == GRAPH_SIDE_J ? 36 : 0);
            gg = base + 108 + (kind == GRAPH_SIDE_J ? 6 : 0);
        }
#pragma unroll
        for (int a = 0; a < 36; ++a) acc[a] = acc[a] + H[a];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[36 + a] = acc[36 + a] + gg[a];
    }
}

__global__ __launch_bounds__(GB) void graph_gather_kernel(GraphView g, double* __restrict__ Hd, double* __restrict__ grad) {
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    if (i >= g.n) return;
    const bool fixed = g.fixed[i] != 0;
    if (!fixed && g.start[i + 1] - g.start[i] > GRAPH_WAVE_LIST) return;   // graph_gather_long_kernel's
    double acc[42];
#pragma unroll
    for (int a = 0; a < 42; ++a) acc[a] = 0.0;
    if (!fixed) diag_terms(g, i, 0, 1, acc);
#pragma unroll
    for (int a = 0; a < 36; ++a) Hd[(size_t)i * 36 + a] = acc[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) grad[(size_t)i * 6 + a] = acc[36 + a];
}

// one wavefront per long node
__global__ __launch_bounds__(GB) void graph_gather_long_kernel(GraphView g, const uint32_t* __restrict__ long_nodes, uint32_t n_long,
                                                               double* __restrict__ Hd, double* __restrict__ grad) {
    const uint32_t w = blockIdx.x * (GB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_long) return;   // (whole wavefronts leave together)
    const uint32_t i = long_nodes[w];
    double acc[42];
#pragma unroll
    for (int a = 0; a < 42; ++a) acc[a] = 0.0;
    diag_terms(g, i, lane, 64, acc);
#pragma unroll
    for (int a = 0; a < 42; ++a) acc[a] = wave_sum(acc[a]);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 36; ++a) Hd[(size_t)i * 36 + a] = acc[a];
#pragma unroll
        for (int a = 0; a < 6; ++a) grad[(size_t)i * 6 + a] = acc[36 + a];
    }
}

// the block of H + lambda diag H of node i
__device__ __forceinline__ void damped_block(const double* __restrict__ Hd, uint32_t i, double lambda, double* M) {
#pragma unroll
    for (int a = 0; a < 36; ++a) M[a] = Hd[(size_t)i * 36 + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) M[a * 7] = M[a * 7] + lambda * M[a * 7];
}

__global__ __launch_bounds__(GB) void graph_precond_kernel(const double* __restrict__ Hd, const uint8_t* __restrict__ fixed, uint32_t n,
                                                           double lambda, double* __restrict__ Minv) {
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    if (i >= n) return;
    double M[36], Mi[36];
    if (fixed[i]) {
        for (int a = 0; a < 36; ++a) Mi[a] = 0.0;
    } else {
        damped_block(Hd, i, lambda, M);
        graph_block_inverse(M, Mi);
    }
    for (int a = 0; a < 36; ++a) Minv[(size_t)i * 36 + a] = Mi[a];
}

// d = 0, r = -g, z = Minv r, p = z; the partials of r^T z
__global__ __launch_bounds__(GB) void pcg_init_kernel(const double* __restrict__ grad, const double* __restrict__ Minv, uint32_t n,
                                                      double* __restrict__ d, double* __restrict__ r, double* __restrict__ z,
                                                      double* __restrict__ p, double* __restrict__ part) {
    __shared__ double sh[GB / 64];
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    double dot = 0.0;
    if (i < n) {
        double rr[6], zz[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) rr[a] = -grad[(size_t)i * 6 + a];
        gr_av6(Minv + (size_t)i * 36, rr, zz);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            d[(size_t)i * 6 + a] = 0.0;
            r[(size_t)i * 6 + a] = rr[a];
            z[(size_t)i * 6 + a] = zz[a];
            p[(size_t)i * 6 + a] = zz[a];
            dot = dot + rr[a] * zz[a];
        }
    }
    const double t = block_fold<false>(dot, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one workgroup: r^T z of the start, and whether there is anything to solve
__global__ __launch_bounds__(GB) void pcg_begin_kernel(const double* __restrict__ part, uint32_t nb, GraphScalars* __restrict__ sc) {
    __shared__ double sh[GB / 64];
    const double rz = fold_partials<false>(part, nb, sh);
    if (threadIdx.x == 0) {
        sc->rz[0] = rz;
        sc->rz[1] = rz;
        sc->rz0 = rz;
        sc->alpha[0] = sc->alpha[1] = 0.0;
        sc->stop[0] = sc->stop[1] = !(rz > 0.0 && rz < INFINITY) ? 1u : 0u;
        sc->iters = 0;
    }
}

// acc (6) += the off-diagonal blocks of the entries off, off + stride, ... times p of the other end
__device__ __forceinline__ void spmv_terms(const GraphView& g, uint32_t node, uint32_t off, uint32_t stride, const double* __restrict__ p,
                                           double* acc) {
    const uint32_t b = g.start[node], e = g.start[node + 1];
    for (uint32_t k = b + off; k < e; k += stride) {
        const uint32_t it = g.items[k], id = it >> 2, kind = it & 3u;
        if (kind == GRAPH_PRIOR) continue;
        const double* Hij = g.elin + (size_t)id * GRAPH_EDGE_LIN + 72;
        const uint32_t other = g.ij[2 * id + (kind == GRAPH_SIDE_I ? 1 : 0)];
        double q[6], t[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) q[a] = p[(size_t)other * 6 + a];
        if (kind == GRAPH_SIDE_I) gr_av6(Hij, q, t);
        else gr_atv6(Hij, q, t);
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = acc[a] + t[a];
    }
}

// wavefront per long node: Ap of it (the diagonal term first, then the folded list)
__global__ __launch_bounds__(GB) void pcg_spmv_long_kernel(GraphView g, const uint32_t* __restrict__ long_nodes, uint32_t n_long,
                                                           const double* __restrict__ Hd, double lambda, const double* __restrict__ p,
                                                           double* __restrict__ Ap, const GraphScalars* __restrict__ sc, int k) {
    if (sc->stop[k & 1]) return;
    const uint32_t w = blockIdx.x * (GB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_long) return;
    const uint32_t i = long_nodes[w];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    spmv_terms(g, i, lane, 64, p, acc);
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] = wave_sum(acc[a]);
    if (lane == 0) {
        double M[36], q[6], y[6];
        damped_block(Hd, i, lambda, M);
#pragma unroll
        for (int a = 0; a < 6; ++a) q[a] = p[(size_t)i * 6 + a];
        gr_av6(M, q, y);
#pragma unroll
        for (int a = 0; a < 6; ++a) Ap[(size_t)i * 6 + a] = y[a] + acc[a];
    }
}

// Ap = (H + lambda diag H) p by block rows, and the partials of p^T A p
__global__ __launch_bounds__(GB) void pcg_spmv_kernel(GraphView g, const double* __restrict__ Hd, double lambda, const double* __restrict__ p,
                                                      double* __restrict__ Ap, double* __restrict__ part, const GraphScalars* __restrict__ sc,
                                                      int k) {
    __shared__ double sh[GB / 64];
    if (sc->stop[k & 1]) return;   // (uniform over the launch)
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    double dot = 0.0;
    if (i < g.n) {
        double y[6], q[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) q[a] = p[(size_t)i * 6 + a];
        if (g.fixed[i]) {
#pragma unroll
            for (int a = 0; a < 6; ++a) Ap[(size_t)i * 6 + a] = y[a] = 0.0;
        } else if (g.start[i + 1] - g.start[i] > GRAPH_WAVE_LIST) {
#pragma unroll
            for (int a = 0; a < 6; ++a) y[a] = Ap[(size_t)i * 6 + a];   // pcg_spmv_long_kernel's, launched before this one
        } else {
            double M[36];
            damped_block(Hd, i, lambda, M);
            gr_av6(M, q, y);
            spmv_terms(g, i, 0, 1, p, y);
#pragma unroll
            for (int a = 0; a < 6; ++a) Ap[(size_t)i * 6 + a] = y[a];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) dot = dot + q[a] * y[a];
    }
    const double t = block_fold<false>(dot, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// alpha = r^T z / p^T A p; d += alpha p, r -= alpha Ap, z = Minv r; the partials of the new r^T z
__global__ __launch_bounds__(GB) void pcg_update_kernel(uint32_t n, uint32_t nb, const double* __restrict__ part_pAp, const double* __restrict__ Minv,
                                                        const double* __restrict__ p, const double* __restrict__ Ap, double* __restrict__ d,
                                                        double* __restrict__ r, double* __restrict__ z, double* __restrict__ part_rz,
                                                        GraphScalars* __restrict__ sc, int k) {
    __shared__ double sh[GB / 64];
    if (sc->stop[k & 1]) return;
    const double pAp = fold_partials<false>(part_pAp, nb, sh);
    const double alpha = (pAp > 0.0 && pAp < INFINITY) ? sc->rz[k & 1] / pAp : 0.0;
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    double dot = 0.0;
    if (i < n) {
        double rr[6], zz[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            d[(size_t)i * 6 + a] = d[(size_t)i * 6 + a] + alpha * p[(size_t)i * 6 + a];
            rr[a] = r[(size_t)i * 6 + a] - alpha * Ap[(size_t)i * 6 + a];
            r[(size_t)i * 6 + a] = rr[a];
        }
        gr_av6(Minv + (size_t)i * 36, rr, zz);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            z[(size_t)i * 6 + a] = zz[a];
            dot = dot + rr[a] * zz[a];
        }
    }
    const double t = block_fold<false>(dot, sh);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = t;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha[k & 1] = alpha;
}

// beta = (r^T z)_new / r^T z, the stop test, p = z + beta p
__global__ __launch_bounds__(GB) void pcg_direction_kernel(uint32_t n, uint32_t nb, const double* __restrict__ part_rz, const double* __restrict__ z,
                                                           double* __restrict__ p, GraphScalars* __restrict__ sc, int k, double tol2) {
    __shared__ double sh[GB / 64];
    const int cur = k & 1, nxt = cur ^ 1;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (sc->stop[cur]) {
        if (lead) {
            sc->stop[nxt] = 1u;
            sc->rz[nxt] = sc->rz[cur];
        }
        return;
    }
    const double rzn = fold_partials<false>(part_rz, nb, sh);
    const double rz = sc->rz[cur], alpha = sc->alpha[cur];
    const bool broke = !(alpha != 0.0);
    const bool stop = broke || !(rzn > tol2 * sc->rz0) || !(rzn < INFINITY);
    if (!stop) {
        const double beta = rzn / rz;
        const uint32_t i = blockIdx.x * GB + threadIdx.x;
        if (i < n) {
#pragma unroll
            for (int a = 0; a < 6; ++a) p[(size_t)i * 6 + a] = z[(size_t)i * 6 + a] + beta * p[(size_t)i * 6 + a];
        }
    }
    if (lead) {
        sc->rz[nxt] = rzn;
        sc->stop[nxt] = stop ? 1u : 0u;
        if (!broke) sc->iters = sc->iters + 1;
    }
}

__global__ __launch_bounds__(GB) void graph_retract_kernel(const lv_graph_pose* __restrict__ x, const double* __restrict__ d,
                                                           const uint8_t* __restrict__ fixed, uint32_t n, lv_graph_pose* __restrict__ xt,
                                                           double* __restrict__ part) {
    __shared__ double sh[GB / 64];
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    double m = 0.0;
    if (i < n) {
        if (fixed[i]) {
            xt[i] = x[i];
        } else {
            double dd[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                dd[a] = d[(size_t)i * 6 + a];
                const double v = fabs(dd[a]);
                m = v > m ? v : m;
            }
            lv_graph_pose o;
            graph_retract(x[i], dd, &o);
            xt[i] = o;
        }
    }
    const double t = block_fold<true>(m, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one workgroup: *out = scale * (sum or max of the partials)
template <bool MAX>
__global__ __launch_bounds__(GB) void graph_fold_kernel(const double* __restrict__ part, uint32_t nb, double scale, double* __restrict__ out) {
    __shared__ double sh[GB / 64];
    const double t = fold_partials<MAX>(part, nb, sh);
    if (threadIdx.x == 0) *out = scale * t;
}

__global__ __launch_bounds__(GB) void graph_warp_delta_kernel(const lv_graph_pose* __restrict__ now, const lv_graph_pose* __restrict__ x0,
                                                              uint32_t n, double* __restrict__ D) {
    const uint32_t i = blockIdx.x * GB + threadIdx.x;
    if (i >= n) return;
    double m[12];
    graph_warp_delta(now[i], x0[i], m);
    for (int a = 0; a < 12; ++a) D[(size_t)i * 12 + a] = m[a];
}

__global__ __launch_bounds__(GB) void graph_warp_kernel(const float* __restrict__ pts, const uint32_t* __restrict__ keys, size_t count,
                                                        const double* __restrict__ D, float* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * GB + threadIdx.x;
    if (k >= count) return;
    double m[12];
    const double* src = D + (size_t)keys[k] * 12;
    for (int a = 0; a < 12; ++a) m[a] = src[a];
    const float p[3] = {pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]};
    float o[3];
    graph_warp_point(m, p, o);
    out[3 * k] = o[0];
    out[3 * k + 1] = o[1];
    out[3 * k + 2] = o[2];
}

}  // namespace

int GraphStore::assign(hipStream_t stream, const lv_graph_pose* poses, size_t nn, const uint8_t* fixed, const lv_graph_edge* edges, size_t ne,
                       const lv_graph_prior* priors, size_t np) {
    // host side first: the lists, the flags, the long nodes
    std::vector<uint32_t> start(nn + 1), items(2 * ne + np), ij(2 * ne), longs;
    std::vector<uint8_t> fx(nn, 0);
    uint32_t n_fixed = 0;
    if (fixed)
        for (size_t k = 0; k < nn; ++k) n_fixed += (fx[k] = fixed[k] ? 1 : 0);
    const uint32_t longest = graph_incidence(nn, edges, ne, priors, np, start.data(), items.data());
    for (size_t e = 0; e < ne; ++e) {
        ij[2 * e] = edges[e].i;
        ij[2 * e + 1] = edges[e].j;
    }
    for (size_t k = 0; k < nn; ++k)
        if (!fx[k] && start[k + 1] - start[k] > GRAPH_WAVE_LIST) longs.push_back((uint32_t)k);

    LV_HIP(hipStreamSynchronize(stream));   // nothing of the old graph is in flight when its buffers go
    set = false;
    const size_t nf = ne + np, nb = std::max<size_t>(blocks_of(nn, GB), blocks_of(nf, GB));
    int rc = d_x.need(nn);
    if (!rc) rc = d_x0.need(nn);
    if (!rc) rc = d_xt.need(nn);
    if (!rc) rc = d_fixed.need(nn);
    if (!rc) rc = d_edges.need(std::max<size_t>(ne, 1));
    if (!rc) rc = d_priors.need(std::max<size_t>(np, 1));
    if (!rc) rc = d_ij.need(std::max<size_t>(2 * ne, 1));
    if (!rc) rc = d_start.need(nn + 1);
    if (!rc) rc = d_items.need(std::max<size_t>(items.size(), 1));
    if (!rc) rc = d_long.need(std::max<size_t>(longs.size(), 1));
    if (!rc) rc = d_elin.need(std::max<size_t>(ne * GRAPH_EDGE_LIN, 1));
    if (!rc) rc = d_plin.need(std::max<size_t>(np * GRAPH_PRIOR_LIN, 1));
    if (!rc) rc = d_s.need(std::max<size_t>(nf, 1));
    if (!rc) rc = d_Hd.need(nn * 36);
    if (!rc) rc = d_g.need(nn * 6);
    if (!rc) rc = d_Minv.need(nn * 36);
    if (!rc) rc = d_d.need(nn * 6);
    if (!rc) rc = d_r.need(nn * 6);
    if (!rc) rc = d_z.need(nn * 6);
    if (!rc) rc = d_p.need(nn * 6);
    if (!rc) rc = d_Ap.need(nn * 6);
    if (!rc) rc = d_part[0].need(nb);
    if (!rc) rc = d_part[1].need(nb);
    if (!rc) rc = d_scal.need(1);
    if (!rc) rc = h_scal.need(1);
    if (!rc) rc = d_D.need(nn * 12);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_x, poses, nn * sizeof(lv_graph_pose), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_x0, poses, nn * sizeof(lv_graph_pose), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_fixed, fx.data(), nn, hipMemcpyHostToDevice, stream));
    if (ne) LV_HIP(hipMemcpyAsync(d_edges, edges, ne * sizeof(lv_graph_edge), hipMemcpyHostToDevice, stream));
    if (np) LV_HIP(hipMemcpyAsync(d_priors, priors, np * sizeof(lv_graph_prior), hipMemcpyHostToDevice, stream));
    if (ne) LV_HIP(hipMemcpyAsync(d_ij, ij.data(), 2 * ne * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_start, start.data(), (nn + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    if (!items.empty()) LV_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    if (!longs.empty()) LV_HIP(hipMemcpyAsync(d_long, longs.data(), longs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetAsync(d_scal, 0, sizeof(GraphScalars), stream));
    LV_HIP(hipStreamSynchronize(stream));   // (the host vectors above are the copies' sources)
    n = nn;
    n_edges = ne;
    n_priors = np;
    n_long = (uint32_t)longs.size();
    info = lv_graph_info{};
    info.set = 1;
    info.status = -1;
    info.n = (uint32_t)nn;
    info.n_edges = (uint32_t)ne;
    info.n_priors = (uint32_t)np;
    info.n_fixed = n_fixed;
    info.longest_list = longest;
    set = true;
    return LV_OK;
}

// r, s, rho (and in full mode the blocks) of every factor at x; the cost goes to d_scal->cost
int GraphStore::linearise(hipStream_t stream, const lv_graph_pose* x, bool full) {
    const uint32_t nf = (uint32_t)(n_edges + n_priors), nb = blocks_of(nf, GB);
    if (nb) {   // (a graph may hold no factor at all: its cost is 0)
        hipLaunchKernelGGL(graph_linearise_kernel, dim3(nb), dim3(GB), 0, stream, x, d_edges.p, (uint32_t)n_edges, d_priors.p, (uint32_t)n_priors,
                           d_elin.p, d_plin.p, d_s.p, d_part[0].p, full ? 1 : 0);
        LV_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(graph_fold_kernel<false>, dim3(1), dim3(GB), 0, stream, d_part[0].p, nb, 0.5, &d_scal.p->cost);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int GraphStore::read_scalars(hipStream_t stream) {
    LV_HIP(hipMemcpyAsync(h_scal.p, d_scal.p, sizeof(GraphScalars), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int GraphStore::optimise(hipStream_t stream, const lv_graph_params& prm) {
    const uint32_t nn = (uint32_t)n, nbn = blocks_of(n, GB);
    const GraphView g{nn, (uint32_t)n_edges, (uint32_t)n_priors, d_fixed.p, d_ij.p, d_start.p, d_items.p, d_elin.p, d_plin.p};
    const uint32_t nbl = blocks_of(n_long, GB / 64);
    const double tol2 = prm.pcg_tol * prm.pcg_tol;
    double lambda = prm.lambda_init, cost = 0.0;
    uint32_t accepted = 0, rejected = 0, pcg_total = 0;
    double last_step = 0.0;
    int status = LV_GRAPH_MAX_ITERATIONS;
    bool fresh = false;   // the blocks, Hd and g belong to the current poses
    info.status = -1;
    for (int it = 0; it < prm.max_iterations; ++it) {
        if (!fresh) {
            int rc = linearise(stream, d_x, true);
            if (rc) return rc;
            if (n_long) {
                hipLaunchKernelGGL(graph_gather_long_kernel, dim3(nbl), dim3(GB), 0, stream, g, d_long.p, n_long, d_Hd.p, d_g.p);
                LV_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(graph_gather_kernel, dim3(nbn), dim3(GB), 0, stream, g, d_Hd.p, d_g.p);
            LV_HIP(hipGetLastError());
            if (it == 0) {
                rc = read_scalars(stream);
                if (rc) return rc;
                cost = h_scal.p->cost;
                info.initial_cost = cost;
            }
            fresh = true;
        }
        hipLaunchKernelGGL(graph_precond_kernel, dim3(nbn), dim3(GB), 0, stream, d_Hd.p, d_fixed.p, nn, lambda, d_Minv.p);
        LV_HIP(hipGetLastError());
        hipLaunchKernelGGL(pcg_init_kernel, dim3(nbn), dim3(GB), 0, stream, d_g.p, d_Minv.p, nn, d_d.p, d_r.p, d_z.p, d_p.p, d_part[1].p);
        LV_HIP(hipGetLastError());
        hipLaunchKernelGGL(pcg_begin_kernel, dim3(1), dim3(GB), 0, stream, d_part[1].p, nbn, d_scal.p);
        LV_HIP(hipGetLastError());
        for (int k = 0; k < prm.pcg_max_iterations;) {
            const int end = std::min(prm.pcg_max_iterations, k + GRAPH_PCG_CHUNK);
            for (; k < end; ++k) {
                if (n_long) {
                    hipLaunchKernelGGL(pcg_spmv_long_kernel, dim3(nbl), dim3(GB), 0, stream, g, d_long.p, n_long, d_Hd.p, lambda, d_p.p, d_Ap.p,
                                       d_scal.p, k);
                    LV_HIP(hipGetLastError());
                }
                hipLaunchKernelGGL(pcg_spmv_kernel, dim3(nbn), dim3(GB), 0, stream, g, d_Hd.p, lambda, d_p.p, d_Ap.p, d_part[0].p, d_scal.p, k);
                LV_HIP(hipGetLastError());
                hipLaunchKernelGGL(pcg_update_kernel, dim3(nbn), dim3(GB), 0, stream, nn, nbn, d_part[0].p, d_Minv.p, d_p.p, d_Ap.p, d_d.p, d_r.p,
                                   d_z.p, d_part[1].p, d_scal.p, k);
                LV_HIP(hipGetLastError());
                hipLaunchKernelGGL(pcg_direction_kernel, dim3(nbn), dim3(GB), 0, stream, nn, nbn, d_part[1].p, d_z.p, d_p.p, d_scal.p, k, tol2);
                LV_HIP(hipGetLastError());
            }
            if (k >= prm.pcg_max_iterations) break;   // (the scalars are read below in any case)
            const int rc = read_scalars(stream);
            if (rc) return rc;
            if (h_scal.p->stop[k & 1]) break;
        }
        // the trial poses, the step norm and the cost there
        hipLaunchKernelGGL(graph_retract_kernel, dim3(nbn), dim3(GB), 0, stream, d_x.p, d_d.p, d_fixed.p, nn, d_xt.p, d_part[1].p);
        LV_HIP(hipGetLastError());
        hipLaunchKernelGGL(graph_fold_kernel<true>, dim3(1), dim3(GB), 0, stream, d_part[1].p, nbn, 1.0, &d_scal.p->step);
        LV_HIP(hipGetLastError());
        int rc = linearise(stream, d_xt, false);
        if (!rc) rc = read_scalars(stream);
        if (rc) return rc;
        pcg_total += h_scal.p->iters;
        const double cost_new = h_scal.p->cost, step = h_scal.p->step;
        if (step - step == 0.0 && graph_accept(cost_new, cost)) {
            std::swap(d_x, d_xt);
            cost = cost_new;
            fresh = false;
            ++accepted;
            last_step = step;
            lambda = std::max(lambda / 3.0, prm.lambda_min);
            if (step <= prm.step_tol) {
                status = LV_GRAPH_CONVERGED;
                break;
            }
        } else {
            ++rejected;
            lambda = std::min(4.0 * lambda, prm.lambda_max);
        }
    }
    info.status = status;
    info.accepted = accepted;
    info.rejected = rejected;
    info.pcg_iterations = pcg_total;
    info.final_cost = cost;
    info.last_step = last_step;
    info.lambda = lambda;
    return LV_OK;
}

int GraphStore::fetch(hipStream_t stream, lv_graph_pose* poses) {
    LV_HIP(hipMemcpyAsync(poses, d_x.p, n * sizeof(lv_graph_pose), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int GraphStore::chi2(hipStream_t stream, double* edge_s, double* prior_s) {
    const int rc = linearise(stream, d_x, false);
    if (rc) return rc;
    if (edge_s && n_edges) LV_HIP(hipMemcpyAsync(edge_s, d_s.p, n_edges * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (prior_s && n_priors) LV_HIP(hipMemcpyAsync(prior_s, d_s.p + n_edges, n_priors * sizeof(double), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int GraphStore::warp(hipStream_t stream, const void* pts, size_t stride, const uint32_t* keys, size_t count, float* out) {
    if (count == 0) return LV_OK;
    int rc = warp_pts.reserve(stream, count, 3 * 4096);
    if (!rc) rc = d_keys.need_pow2(count, 4096);
    if (!rc) rc = d_out.need_pow2(3 * count, 3 * 4096);
    if (rc) return rc;
    warp_pts.append(pts, stride, count);
    rc = warp_pts.upload(stream);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_keys.p, keys, count * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(graph_warp_delta_kernel, dim3(blocks_of(n, GB)), dim3(GB), 0, stream, d_x.p, d_x0.p, (uint32_t)n, d_D.p);
    LV_HIP(hipGetLastError());
    hipLaunchKernelGGL(graph_warp_kernel, dim3(blocks_of(count, GB)), dim3(GB), 0, stream, warp_pts.d.p, d_keys.p, count, d_D.p, d_out.p);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(out, d_out.p, 3 * count * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

void GraphStore::release() {
    d_x.release(); d_x0.release(); d_xt.release(); d_fixed.release(); d_edges.release(); d_priors.release(); d_ij.release();
    d_start.release(); d_items.release(); d_long.release(); d_elin.release(); d_plin.release(); d_s.release(); d_Hd.release();
    d_g.release(); d_Minv.release(); d_d.release(); d_r.release(); d_z.release(); d_p.release(); d_Ap.release();
    d_part[0].release(); d_part[1].release(); d_scal.release(); h_scal.release(); warp_pts.release(); d_keys.release(); d_D.release();
    d_out.release();
    *this = GraphStore();
}

}  // namespace lv
