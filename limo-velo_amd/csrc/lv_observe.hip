// lv_observe.hip — aiding observations (GPS / barometer position, world or body velocity, ZUPT, AHRS attitude) as measurement
// updates of the resident filter, on the device and in order with the queued predictions: lv_predict ... -> lv_observe ->
// lv_correct never round-trips x, P.  The rule and the summation order of every product: include/limovelo_hip.h "Aiding
// observations" (tests/aiding_ref.py restates it in numpy, tests/test_aiding_ref.py anchors that to 50 digits).
//
// N-independent, latency-only work like predict_kernel: ONE workgroup of 576 lanes; x, P enter LDS once for the whole batch and
// leave it once.  Per observation the scalar manifold part (h, y, the two 3x3 blocks of H, the m x m Cholesky, the gate, [+]) runs
// on single lanes, P H^T on 23 x m lanes, the rows of K on 23 lanes, A, A P and A P A^T + K R K^T on one lane per entry.  H has at
// most two non-zero 3x3 blocks (columns c0[0].., c0[1]..): H P H^T and K H are sums over those six columns, never a dense H.
// Every __syncthreads is at the top level of the loop over the observations, whose trip count is a kernel argument: all 576 lanes
// reach each of them whatever the status of the observation (the work between them is predicated, not the barriers).
#include "lv_host.hpp"
#include "lv_manifold.hpp"

namespace lv {

struct ObserveArgs {
    int n;
    lv_observation obs[LV_OBSERVE_BATCH];
};

// [NS + 1]: a lane per entry reads a row (lanes of a wavefront: stride NS + 1 doubles, odd in 8-byte words) or a column (stride 1)
__global__ __launch_bounds__(576) void observe_kernel(FilterDev* f, ObserveArgs a, lv_observe_result* res) {
    __shared__ double sP[NS][NS + 1], sA[NS][NS + 1], sAP[NS][NS + 1];
    __shared__ double sPHt[NS][3], sK[NS][3], sKR[NS][3], sdx[NS];
    __shared__ double sx[NX];
    __shared__ double sH[2][3][3], sRm[3][3], sy[3], sL[3][3];   // rows of the masked components, in ascending order
    __shared__ int s_status;
    const int tid = threadIdx.x;
    if (tid < NS * NS) sP[tid / NS][tid % NS] = f->P[tid];
    if (tid < NX) sx[tid] = f->x[tid];
    __syncthreads();
    for (int ob = 0; ob < a.n; ++ob) {
        const lv_observation& o = a.obs[ob];
        // uniform: the masked components, and where the blocks of H sit
        int comp[3], m = 0;
        for (int k = 0; k < 3; ++k) if (o.mask >> k & 1) comp[m++] = k;
        for (int k = m; k < 3; ++k) comp[k] = 0;
        const int kind = o.kind;
        const int nblk = (kind == LV_OBS_POSITION || kind == LV_OBS_VELOCITY_BODY) ? 2 : 1;
        const int c0[2] = {kind == LV_OBS_POSITION ? 0 : kind == LV_OBS_ATTITUDE ? 3 : 12, 3};

        if (tid == 0) {   // h, y, the blocks of H
            double R[9], Ha[9], Hb[9], y[3];
            for (int i = 0; i < 9; ++i) { Ha[i] = (i % 4 == 0) ? 1.0 : 0.0; Hb[i] = 0.0; }
            quat_to_rot(sx + 3, R);
            if (kind == LV_OBS_POSITION) {
                double Rl[3], hl[9], RH[9];
                d_mat3_vec(R, o.lever, Rl);
                for (int i = 0; i < 3; ++i) y[i] = o.z[i] - (sx[i] + Rl[i]);
                d_hat3(o.lever, hl);
                d_mat3_mul(R, hl, RH);
                for (int i = 0; i < 9; ++i) Hb[i] = -RH[i];
            } else if (kind == LV_OBS_VELOCITY_WORLD) {
                for (int i = 0; i < 3; ++i) y[i] = o.z[i] - sx[14 + i];
            } else if (kind == LV_OBS_VELOCITY_BODY) {
                double vb[3];
                d_mat3_T(R, Ha);
                d_mat3_vec(Ha, sx + 14, vb);
                for (int i = 0; i < 3; ++i) y[i] = o.z[i] - vb[i];
                d_hat3(vb, Hb);
            } else {
                const double qc[4] = {-sx[3], -sx[4], -sx[5], sx[6]};
                double qe[4];
                d_quat_mul(qc, o.z, qe);
                d_so3_log(qe, y);
            }
            for (int k = 0; k < m; ++k) {
                sy[k] = y[comp[k]];
                for (int j = 0; j < 3; ++j) {
                    sH[0][k][j] = Ha[comp[k] * 3 + j];
                    sH[1][k][j] = Hb[comp[k] * 3 + j];
                    sRm[k][j] = j < m ? o.R[comp[k] * 3 + comp[j]] : 0.0;
                }
            }
            res[ob].rows = m;
            for (int i = 0; i < 3; ++i) res[ob].y[i] = y[i];
        }
        __syncthreads();
        if (tid < NS * m) {   // P H^T
            const int i = tid / m, k = tid % m;
            double s = 0.0;
            for (int b = 0; b < nblk; ++b)
                for (int j = 0; j < 3; ++j) s += sP[i][c0[b] + j] * sH[b][k][j];
            sPHt[i][k] = s;
        }
        __syncthreads();
        if (tid == 0) {   // S, its Cholesky factor, the gate
            double S[3][3], L[3][3], w[3] = {0.0, 0.0, 0.0};
            int status = 0;
            for (int k = 0; k < m; ++k)
                for (int l = 0; l <= k; ++l) {
                    double s = 0.0;
                    for (int b = 0; b < nblk; ++b)
                        for (int j = 0; j < 3; ++j) s += sH[b][k][j] * sPHt[c0[b] + j][l];
                    S[k][l] = s + sRm[k][l];
                }
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) L[i][j] = 0.0;
            for (int j = 0; j < m && status == 0; ++j) {
                double d = S[j][j];
                for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
                if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) { status = 2; break; }
                L[j][j] = sqrt(d);
                for (int i = j + 1; i < m; ++i) {
                    double t = S[i][j];
                    for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
                    L[i][j] = t / L[j][j];
                }
            }
            double nis = 0.0;
            if (status == 0) {
                for (int i = 0; i < m; ++i) {
                    double t = sy[i];
                    for (int k = 0; k < i; ++k) t -= L[i][k] * w[k];
                    w[i] = t / L[i][i];
                }
                for (int i = 0; i < m; ++i) nis += w[i] * w[i];
                if (o.gate > 0.0 && nis > o.gate) status = 1;
            }
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) sL[i][j] = L[i][j];
            s_status = status;
            res[ob].status = status;
            res[ob].nis = nis;
        }
        __syncthreads();
        const bool ok = s_status == 0;
        if (ok && tid < NS) {   // row tid of K = P H^T S^-1, of dx = K y and of K R
            const int i = tid;
            double t[3] = {0.0, 0.0, 0.0}, K[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < m; ++k) {
                double v = sPHt[i][k];
                for (int l = 0; l < k; ++l) v -= sL[k][l] * t[l];
                t[k] = v / sL[k][k];
            }
            for (int k = m - 1; k >= 0; --k) {
                double v = t[k];
                for (int l = k + 1; l < m; ++l) v -= sL[l][k] * K[l];
                K[k] = v / sL[k][k];
            }
            double d = 0.0;
            for (int k = 0; k < m; ++k) d += K[k] * sy[k];
            sdx[i] = d;
            for (int l = 0; l < 3; ++l) {
                double s = 0.0;
                for (int k = 0; k < m; ++k) s += K[k] * sRm[k][l];
                sKR[i][l] = s;
                sK[i][l] = l < m ? K[l] : 0.0;
            }
        }
        __syncthreads();
        if (ok && tid < NS * NS) {   // A = I - K H
            const int i = tid / NS, c = tid % NS;
            double v = i == c ? 1.0 : 0.0;
            for (int b = 0; b < nblk; ++b)
                if (c >= c0[b] && c < c0[b] + 3) {
                    double s = 0.0;
                    for (int k = 0; k < m; ++k) s += sK[i][k] * sH[b][k][c - c0[b]];
                    v = (i == c ? 1.0 : 0.0) - s;
                }
            sA[i][c] = v;
        }
        if (ok && tid == 544) {   // x [+] dx (a lane of the wavefront with the fewest entries of A)
            double x[NX], dx[NS];
            for (int i = 0; i < NX; ++i) x[i] = sx[i];
            for (int i = 0; i < NS; ++i) dx[i] = sdx[i];
            d_state_boxplus(x, dx);
            for (int i = 0; i < NX; ++i) sx[i] = x[i];
        }
        __syncthreads();
        if (ok && tid < NS * NS) {   // A P
            const int i = tid / NS, j = tid % NS;
            double s = 0.0;
            for (int c = 0; c < NS; ++c) s += sA[i][c] * sP[c][j];
            sAP[i][j] = s;
        }
        __syncthreads();
        if (ok && tid < NS * NS) {   // (A P) A^T + (K R) K^T, the upper triangle mirrored
            const int i = tid / NS, j = tid % NS;
            if (i <= j) {
                double s = 0.0, q = 0.0;
                for (int c = 0; c < NS; ++c) s += sAP[i][c] * sA[j][c];
                for (int l = 0; l < m; ++l) q += sKR[i][l] * sK[j][l];
                const double v = s + q;
                sP[i][j] = v;
                sP[j][i] = v;
            }
        }
        __syncthreads();   // (the next observation reads sx, sP; lane 0 rewrites sH, sy)
    }
    if (tid < NS * NS) f->P[tid] = sP[tid / NS][tid % NS];
    if (tid < NX) f->x[tid] = sx[tid];
}

int launch_observe(hipStream_t stream, FilterDev* f, const lv_observation* obs, int n, lv_observe_result* d_results) {
    if (n <= 0) return LV_OK;
    ObserveArgs a{};
    a.n = n < LV_OBSERVE_BATCH ? n : LV_OBSERVE_BATCH;
    for (int i = 0; i < a.n; ++i) a.obs[i] = obs[i];
    hipLaunchKernelGGL(observe_kernel, dim3(1), dim3(576), 0, stream, f, a, d_results);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

}  // namespace lv
