// MI355X-native Optimizer::OptimizeSim3 (Optimizer.cc:1405-1637), the fourth step of
// LoopClosing::ComputeSim3 (LoopClosing.cc:441-449).
//
// One 256-thread workgroup per slot runs the whole two-stage solve on the device: optimize(5),
// the chi2 > th2 removal on g2o's stale _error, the `nCorrespondences - nBad < 10` exit, then
// optimize(nBad > 0 ? 10 : 5) and the final count. The graph has one free vertex, the 7-DoF
// VertexSim3Expmap (types_seven_dof_expmap.h:48-94); every pair contributes an EdgeSim3ProjectXYZ
// and an EdgeInverseSim3ProjectXYZ (:130-171) whose point vertices are fixed. Their analytic
// linearizeOplus is commented out in the reference, so g2o differentiates numerically
// (base_binary_edge.hpp:131-205): central differences at delta = 1e-9 through oplus = Sim3(update)
// * estimate. The 14 perturbed estimates (12 under _fix_scale, whose column is exactly zero) and
// their inverses are the same for every edge of a linearisation, so lanes 0..13 build them into LDS
// once per LM iteration; every thread then walks its pairs (pair k, k + 256, ...):
//   per LM iteration   base errors, 2 x 14 perturbed errors, Huber weights, J^T W J / J^T W e
//                      partials per thread; one fixed-tree block reduction of 1 + 28 + 7 doubles
//   per LM trial       thread 0: Eigen::LDLT (diagonal pivoting) of H + lambda I at dimension 7,
//                      Sim3(update) * estimate; all threads: trial errors (kept as the stale
//                      _error) + robust chi2 reduction; thread 0: accept / reject
// The Levenberg-Marquardt control is that of pose_opt_kernel (orb_pose.hip), restated from
// optimization_algorithm_levenberg.cpp. All FP64, no floating-point atomics, every loop bounded.
// None of the Sim3 paths normalises a quaternion (sim3.h:64-67, 136, 233-272).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orb_engine.h"
#include "orbslam2_amd.h"
#include "se3_device.h"

using namespace orbamd;
using namespace g2oamd;

#define SO_CHK(x)                                                                   \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "orbslam2_amd sim3opt: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return ORBX_EDEVICE;                                                    \
        }                                                                           \
    } while (0)

namespace orbsim3opt {

constexpr int kThreads = 256;
constexpr int kRed = 36;    // chi2 + 28 (lower H) + 7 (b)
constexpr int kMaxPairs = 1 << 20;

struct Sim3 { double q[4]; double t[3]; double s; };   // q = (x, y, z, w), never normalised

struct SlotHdr {
    int n, fix_scale;
    float th2, pad;
    double delta;          // (double)(float)sqrt(th2): deltaHuber (Optimizer.cc:1464)
    double K1[4], K2[4];   // fx fy cx cy, widened from float (:1439-1446)
    Sim3 S;                // g2oS12
};

struct Slots {
    const SlotHdr *hdr;
    const float4 *pts;     // [S][cap][3]: (X1c, invSigma2_1) (X2c, invSigma2_2) (obs1, obs2)
    double *err;           // [S][cap][4] g2o _error of e12, e21
    uint8_t *state;        // [S][cap]
    double *chi2;          // [S][cap][2]
    double *Sout;          // [S][8]
    int *nin;              // [S]
    int *iters;            // [S][2]
    int cap;
};

// Eigen::Quaterniond(const Matrix3d &) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl),
// as it stands: no normalisation, no sign choice. Branches spelled out per pivot so that no local
// array is indexed dynamically.
__device__ inline void quat_from_R(const double m[9], double q[4]) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > (i == 0 ? m[0] : m[4])) i = 2;
        if (i == 0) {
            t = sqrt(m[0] - m[4] - m[8] + 1.0);
            q[0] = 0.5 * t;
            t = 0.5 / t;
            q[3] = (m[7] - m[5]) * t;
            q[1] = (m[3] + m[1]) * t;
            q[2] = (m[6] + m[2]) * t;
        } else if (i == 1) {
            t = sqrt(m[4] - m[8] - m[0] + 1.0);
            q[1] = 0.5 * t;
            t = 0.5 / t;
            q[3] = (m[2] - m[6]) * t;
            q[2] = (m[7] + m[5]) * t;
            q[0] = (m[1] + m[3]) * t;
        } else {
            t = sqrt(m[8] - m[0] - m[4] + 1.0);
            q[2] = 0.5 * t;
            t = 0.5 / t;
            q[3] = (m[3] - m[1]) * t;
            q[0] = (m[2] + m[6]) * t;
            q[1] = (m[5] + m[7]) * t;
        }
    }
}

// Sim3(const Vector7d &update) (sim3.h:70-142): (omega, upsilon, sigma), all four branches
__device__ inline Sim3 sim3_exp(const double u[7]) {
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double O[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double O2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    Sim3 r;
    r.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, Cc, ra = 1.0, rb = 1.0;   // R = I + ra Omega + rb Omega2 (ra = rb = 1: the small-angle form)
    if (fabs(sigma) < eps) {
        Cc = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
            ra = sin(theta) / theta;
            rb = (1 - cos(theta)) / (theta * theta);
        }
    } else {
        Cc = (r.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * r.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * r.s) / (sigma2 * sigma);
        } else {
            ra = sin(theta) / theta;
            rb = (1 - cos(theta)) / (theta * theta);
            const double a = r.s * sin(theta), b = r.s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (Cc - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    double R[9], W[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = i % 4 == 0 ? 1.0 : 0.0;
        R[i] = I + ra * O[i] + rb * O2[i];
        W[i] = A * O[i] + B * O2[i] + Cc * I;
    }
    quat_from_R(R, r.q);
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    return r;
}

// Sim3::operator* (sim3.h:266-272)
__device__ inline Sim3 sim3_mul(const Sim3 &a, const Sim3 &b) {
    Sim3 r;
    r.q[3] = a.q[3] * b.q[3] - a.q[0] * b.q[0] - a.q[1] * b.q[1] - a.q[2] * b.q[2];
    r.q[0] = a.q[3] * b.q[0] + a.q[0] * b.q[3] + a.q[1] * b.q[2] - a.q[2] * b.q[1];
    r.q[1] = a.q[3] * b.q[1] + a.q[1] * b.q[3] + a.q[2] * b.q[0] - a.q[0] * b.q[2];
    r.q[2] = a.q[3] * b.q[2] + a.q[2] * b.q[3] + a.q[0] * b.q[1] - a.q[1] * b.q[0];
    double rt[3];
    quat_rotate(a.q, b.t, rt);
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

// Sim3::inverse (sim3.h:233-236)
__device__ inline Sim3 sim3_inverse(const Sim3 &a) {
    Sim3 r;
    r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
    const double f = -1. / a.s;
    const double v[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    quat_rotate(r.q, v, r.t);
    r.s = 1. / a.s;
    return r;
}

// computeError of either edge (types_seven_dof_expmap.h:138-145, 160-167) with the Sim3 the
// vertex holds (e12) or its inverse (e21): obs - cam_map(project(S.map(X)))
__device__ inline void edge_error(const Sim3 &S, const double K[4], const double X[3], double ou, double ov, double e[2]) {
    double p[3];
    quat_rotate(S.q, X, p);
    p[0] = S.s * p[0] + S.t[0];
    p[1] = S.s * p[1] + S.t[1];
    p[2] = S.s * p[2] + S.t[2];
    e[0] = ou - (p[0] / p[2] * K[0] + K[2]);
    e[1] = ov - (p[1] / p[2] * K[1] + K[3]);
}

__device__ inline double edge_chi2(const double e[2], double info) { return e[0] * info * e[0] + e[1] * info * e[1]; }

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-90): rho0, weight rho1
__device__ inline double huber(double chi, double delta, double &w) {
    w = 1.0;
    const double dsqr = delta * delta;
    if (chi <= dsqr) return chi;
    const double s = sqrt(chi);
    w = delta / s;
    return 2 * s * delta - dsqr;
}

// sum-reduce v[0..N) over the workgroup into red[] with a fixed tree (every thread reads the result)
template <int N>
__device__ inline void block_reduce(double *v, double *red, double (*wsum)[kRed]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        v[k] = x;
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < N; k++) wsum[wv][k] = v[k];
    __syncthreads();
    if (threadIdx.x < N) red[threadIdx.x] = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) +
                                            wsum[3][threadIdx.x];
    __syncthreads();
}

// Eigen::LDLT<MatrixXd> (lower, diagonal pivoting) + solve at dimension 7; false when
// !isPositive() (linear_solver_dense.h:104-112). The register-resident form of orb_pose.hip's
// ldlt_solve6: the matrix is kept fully symmetric, so Eigen's partial lower-triangle swap of pivot
// k <-> big equals a full symmetric row + column swap with compile-time indices.
__device__ bool ldlt_solve7(const double *Hin, const double *b, double *x) {
    constexpr int D = 7;
    double a[D][D];
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
        for (int j = 0; j < D; j++) a[i][j] = i >= j ? Hin[D * i + j] : Hin[D * j + i];
    int tr[D];
    int sign = 0;
    bool fail = false;
#pragma unroll
    for (int k = 0; k < D; k++) {
        int big = k;
        double bv = fabs(a[k][k]);
#pragma unroll
        for (int i = k + 1; i < D; i++)
            if (fabs(a[i][i]) > bv) { bv = fabs(a[i][i]); big = i; }
        tr[k] = big;
#pragma unroll
        for (int r = k + 1; r < D; r++) {
            if (r == big) {
#pragma unroll
                for (int j = 0; j < D; j++) { const double t = a[k][j]; a[k][j] = a[r][j]; a[r][j] = t; }
#pragma unroll
                for (int i = 0; i < D; i++) { const double t = a[i][k]; a[i][k] = a[i][r]; a[i][r] = t; }
            }
        }
        if (k > 0) {
            double temp[D];
#pragma unroll
            for (int j = 0; j < k; j++) temp[j] = a[j][j] * a[k][j];
            double s = 0;
#pragma unroll
            for (int j = 0; j < k; j++) s += a[k][j] * temp[j];
            a[k][k] -= s;
#pragma unroll
            for (int i = k + 1; i < D; i++) {
                double t = 0;
#pragma unroll
                for (int j = 0; j < k; j++) t += a[i][j] * temp[j];
                a[i][k] -= t;
                a[k][i] = a[i][k];
            }
        }
        const double akk = a[k][k];
        const bool valid = fabs(akk) > 0;
        if (k == 0 && !valid) fail = true;
        if (valid)
#pragma unroll
            for (int i = k + 1; i < D; i++) { a[i][k] /= akk; a[k][i] = a[i][k]; }
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (fail || !(sign == 1 || sign == 0)) return false;
    double y[D];
#pragma unroll
    for (int i = 0; i < D; i++) y[i] = b[i];
#pragma unroll
    for (int k = 0; k < D; k++)
#pragma unroll
        for (int r = k + 1; r < D; r++)
            if (r == tr[k]) { const double t = y[k]; y[k] = y[r]; y[r] = t; }
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
        for (int j = 0; j < i; j++) y[i] -= a[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < D; i++) y[i] = fabs(a[i][i]) > DBL_MIN ? y[i] / a[i][i] : 0.0;
#pragma unroll
    for (int i = D - 1; i >= 0; i--)
#pragma unroll
        for (int j = i + 1; j < D; j++) y[i] -= a[j][i] * y[j];
#pragma unroll
    for (int k = D - 1; k >= 0; k--)
#pragma unroll
        for (int r = k + 1; r < D; r++)
            if (r == tr[k]) { const double t = y[k]; y[k] = y[r]; y[r] = t; }
#pragma unroll
    for (int i = 0; i < D; i++) x[i] = y[i];
    return true;
}

struct Shared {
    Sim3 T, T2;
    Sim3 P[14], Pi[14];     // oplus(+delta e_d), oplus(-delta e_d) at 2d, 2d + 1, and their inverses
    Sim3 Ti;                // inverse of the estimate the errors are evaluated at
    double J[14][kThreads]; // the Jacobian of the edge a thread is working on: [row * 7 + direction][thread]
    double red[kRed];
    double wsum[4][kRed];
    double H[49], b[7];
    double Hl[49], x[7];
    double lambda, ni, currentChi, iniChi, rho;
    int qmax, nBad, stop, cnt;
};

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69)
__device__ inline Sim3 sim3_oplus(const Sim3 &T, const double *x, bool fix_scale) {
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = x[k];
    if (fix_scale) u[6] = 0;
    return sim3_mul(sim3_exp(u), T);
}

// errors of the active pairs at `T` (inverse in sh.Ti) + the robust chi2 partial; with `lin` also
// the numeric Jacobians from sh.P / sh.Pi and the H / b partials
template <bool lin>
__device__ void accumulate(const Slots &P, int s, const SlotHdr &h, const Sim3 &T, Shared &sh) {
    double v[kRed];
#pragma unroll
    for (int k = 0; k < kRed; k++) v[k] = 0;
    const long long base = (long long)s * P.cap;
    const bool fix = h.fix_scale != 0;
    const double scalar = 1.0 / (2 * 1e-9);
    for (int k = threadIdx.x; k < h.n; k += kThreads) {
        if (P.state[base + k]) continue;
        const float4 a = P.pts[(base + k) * 3], b = P.pts[(base + k) * 3 + 1], c = P.pts[(base + k) * 3 + 2];
        double *E = P.err + (base + k) * 4;
        // rolled on purpose: two edges x 14 perturbed errors unrolled keep every LDS estimate live at
        // once and spill; the Jacobian goes through this thread's LDS column so no register array is
        // indexed by the direction
#pragma unroll 1
        for (int edge = 0; edge < 2; edge++) {   // 0: e12 (EdgeSim3ProjectXYZ), 1: e21 (EdgeInverseSim3ProjectXYZ)
            const double X[3] = {edge ? a.x : b.x, edge ? a.y : b.y, edge ? a.z : b.z};
            const double *K = edge ? h.K2 : h.K1;
            const double ou = edge ? c.z : c.x, ov = edge ? c.w : c.y;
            const double info = edge ? b.w : a.w;
            double e[2];
            edge_error(edge ? sh.Ti : T, K, X, ou, ov, e);
            E[2 * edge] = e[0];
            E[2 * edge + 1] = e[1];
            double w;
            v[0] += huber(edge_chi2(e, info), h.delta, w);
            if constexpr (lin) {
                // BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:176-197), vertex 1
                const Sim3 *Sp = edge ? sh.Pi : sh.P;
                const int nd = fix ? 6 : 7;   // Sim3(0) * S == S bit for bit: the scale column is exactly zero
                sh.J[6][threadIdx.x] = 0;
                sh.J[13][threadIdx.x] = 0;
#pragma unroll 1
                for (int d = 0; d < nd; d++) {
                    double ep[2], em[2];
                    edge_error(Sp[2 * d], K, X, ou, ov, ep);
                    edge_error(Sp[2 * d + 1], K, X, ou, ov, em);
                    sh.J[d][threadIdx.x] = scalar * (ep[0] - em[0]);
                    sh.J[7 + d][threadIdx.x] = scalar * (ep[1] - em[1]);
                }
                double J[14];   // [row][direction]
#pragma unroll
                for (int d = 0; d < 14; d++) J[d] = sh.J[d][threadIdx.x];
                // constructQuadraticForm (:91-113): lower triangle, row-major; constant register indices
                const double W = w * info;
                int u = 1;
#pragma unroll
                for (int r = 0; r < 7; r++)
#pragma unroll
                    for (int q = 0; q <= r; q++) {
                        double hh = J[r] * W * J[q];
                        hh += J[7 + r] * W * J[7 + q];
                        v[u++] += hh;
                    }
#pragma unroll
                for (int r = 0; r < 7; r++) {
                    double t = J[r] * (info * e[0]);
                    t += J[7 + r] * (info * e[1]);
                    v[29 + r] -= w * t;
                }
            }
        }
    }
    if constexpr (lin) block_reduce<kRed>(v, sh.red, sh.wsum);
    else block_reduce<1>(v, sh.red, sh.wsum);
}

// SparseOptimizer::optimize(iterations) + OptimizationAlgorithmLevenberg::solve on the Sim3 vertex
__device__ int optimize(const Slots &P, int s, const SlotHdr &h, int iterations, Shared &sh) {
    const int tid = threadIdx.x;
    const bool fix = h.fix_scale != 0;
    int it = 0;
    for (int i = 0; i < iterations; i++) {
        if (tid < 14) {   // the perturbed estimates of this linearisation and their inverses
            const int d = tid >> 1;
            const double dl = (tid & 1) ? -1e-9 : 1e-9;
            double u[7];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = k == d ? dl : 0.0;
            const Sim3 Sp = sim3_oplus(sh.T, u, fix);
            sh.P[tid] = Sp;
            sh.Pi[tid] = sim3_inverse(Sp);
        } else if (tid == 14) {
            sh.Ti = sim3_inverse(sh.T);
        }
        __syncthreads();
        accumulate<true>(P, s, h, sh.T, sh);
        if (tid == 0) {
            sh.currentChi = sh.iniChi = sh.red[0];
            int u = 1;
            for (int a = 0; a < 7; a++)
                for (int c = 0; c <= a; c++) { sh.H[7 * a + c] = sh.red[u]; sh.H[7 * c + a] = sh.red[u]; u++; }
            for (int a = 0; a < 7; a++) sh.b[a] = sh.red[29 + a];
            if (i == 0) {
                double mx = 0;
                for (int a = 0; a < 7; a++) mx = fmax(fabs(sh.H[8 * a]), mx);
                sh.lambda = 1e-5 * mx;
                sh.ni = 2;
                sh.nBad = 0;
            }
            sh.qmax = 0;
        }
        __syncthreads();
        bool ok2 = true;
        do {
            if (tid == 0) {
                for (int k = 0; k < 49; k++) sh.Hl[k] = sh.H[k];
                for (int a = 0; a < 7; a++) sh.Hl[8 * a] += sh.lambda;
                ok2 = ldlt_solve7(sh.Hl, sh.b, sh.x);
                if (fix) sh.x[6] = 0;                     // oplusImpl writes update[6] = 0 into the solver's x
                sh.T2 = sim3_oplus(sh.T, sh.x, fix);
                sh.Ti = sim3_inverse(sh.T2);
            }
            __syncthreads();
            accumulate<false>(P, s, h, sh.T2, sh);
            if (tid == 0) {
                double tempChi = sh.red[0];
                if (!ok2) tempChi = DBL_MAX;
                double rho = sh.currentChi - tempChi;
                double scale = 0;
                for (int a = 0; a < 7; a++) scale += sh.x[a] * (sh.lambda * sh.x[a] + sh.b[a]);
                scale += 1e-3;
                rho /= scale;
                if (rho > 0 && isfinite(tempChi)) {
                    double alpha = 1. - pow((2 * rho - 1), 3);
                    alpha = fmin(alpha, 2. / 3.);
                    sh.lambda *= fmax(1. / 3., alpha);
                    sh.ni = 2;
                    sh.currentChi = tempChi;
                    sh.T = sh.T2;                       // discardTop
                } else {
                    sh.lambda *= sh.ni;                 // pop: the edges keep the trial _error
                    sh.ni *= 2;
                }
                sh.rho = rho;
                sh.qmax++;
            }
            __syncthreads();
        } while (sh.rho < 0 && sh.qmax < 10);
        it++;
        if (tid == 0) {
            bool ok = true;
            if (sh.qmax == 10 || sh.rho == 0) ok = false;
            else {
                if ((sh.iniChi - sh.currentChi) * 1e3 < sh.iniChi) sh.nBad++; else sh.nBad = 0;
                if (sh.nBad >= 3) ok = false;
            }
            sh.stop = ok ? 0 : 1;
        }
        __syncthreads();
        if (sh.stop) break;
    }
    return it;
}

// the chi2() > th2 test of :1583 / :1622 on the stale _error of the active pairs: a failing pair gets
// `mark`; returns the number of failing pairs of the slot
__device__ int check_pairs(const Slots &P, int s, const SlotHdr &h, uint8_t mark, Shared &sh) {
    const int tid = threadIdx.x;
    const long long base = (long long)s * P.cap;
    const double th2 = h.th2;
    int bad = 0;
    for (int k = tid; k < h.n; k += kThreads) {
        if (P.state[base + k]) continue;
        const double *E = P.err + (base + k) * 4;
        const double e12[2] = {E[0], E[1]}, e21[2] = {E[2], E[3]};
        const double c12 = edge_chi2(e12, P.pts[(base + k) * 3].w), c21 = edge_chi2(e21, P.pts[(base + k) * 3 + 1].w);
        if (c12 > th2 || c21 > th2) {
            P.state[base + k] = mark;
            bad++;
        }
    }
    __syncthreads();
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
    atomicAdd(&sh.cnt, bad);
    __syncthreads();
    return sh.cnt;
}

__global__ __launch_bounds__(kThreads) void sim3_opt_kernel(Slots P) {
    __shared__ Shared sh;
    const int s = blockIdx.x, tid = threadIdx.x;
    const SlotHdr &h = P.hdr[s];
    const long long base = (long long)s * P.cap;
    for (int k = tid; k < h.n; k += kThreads) P.state[base + k] = 0;
    if (tid < 4) P.Sout[8 * s + tid] = h.S.q[tid];      // `return 0` leaves g2oS12 as it came
    else if (tid < 7) P.Sout[8 * s + tid] = h.S.t[tid - 4];
    else if (tid == 7) P.Sout[8 * s + 7] = h.S.s;
    if (tid < 2) P.iters[2 * s + tid] = -1;
    if (tid == 0) {
        P.nin[s] = 0;
        sh.T = h.S;                                       // vSim3->setEstimate(g2oS12)
        for (int k = 0; k < 7; k++) sh.x[k] = 0;          // the solver's x starts at zero
    }
    if (h.n <= 0) return;
    __syncthreads();
    const int it1 = optimize(P, s, h, 5, sh);             // :1571
    const int nBad = check_pairs(P, s, h, 1, sh);         // :1575-1595
    if (tid == 0) P.iters[2 * s] = it1;
    int nIn = 0;
    if (h.n - nBad >= 10) {                               // :1605
        const int it2 = optimize(P, s, h, nBad > 0 ? 10 : 5, sh);   // :1598-1611
        const int nOut = check_pairs(P, s, h, 2, sh);     // :1614-1629
        nIn = h.n - nBad - nOut;
        if (tid == 0) {
            P.iters[2 * s + 1] = it2;
            P.nin[s] = nIn;
#pragma unroll
            for (int k = 0; k < 4; k++) P.Sout[8 * s + k] = sh.T.q[k];   // g2oS12 = vSim3_recov->estimate()
#pragma unroll
            for (int k = 0; k < 3; k++) P.Sout[8 * s + 4 + k] = sh.T.t[k];
            P.Sout[8 * s + 7] = sh.T.s;
        }
    }
    for (int k = tid; k < h.n; k += kThreads) {           // the last chi2() of every pair, removed ones included
        const double *E = P.err + (base + k) * 4;
        const double e12[2] = {E[0], E[1]}, e21[2] = {E[2], E[3]};
        P.chi2[(base + k) * 2] = edge_chi2(e12, P.pts[(base + k) * 3].w);
        P.chi2[(base + k) * 2 + 1] = edge_chi2(e21, P.pts[(base + k) * 3 + 1].w);
    }
}

}  // namespace orbsim3opt

using namespace orbsim3opt;

struct orbo_engine {
    bool dev_ready = false;   // the device is first touched by a call whose arguments passed every check
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    int nslots = 0, cap = 0;
    bool allocated = false;
    std::vector<int> n;       // pairs staged per slot, -1 = never staged
    DevBuf hdr, pts, err, state, chi2, Sout, nin, iters;
    std::vector<float4> tpts;
};

static int ensure_device(orbo_engine *e) {
    if (!e->dev_ready) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return ORBX_EDEVICE;
        if (hipGetDevice(&e->device) != hipSuccess) return ORBX_EDEVICE;
        if (!e->stream && hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return ORBX_EDEVICE;
        if (!e->done && !(e->done = make_done_event())) return ORBX_EDEVICE;
        e->dev_ready = true;
    }
    SO_CHK(hipSetDevice(e->device));
    if (!e->allocated) {
        const size_t S = (size_t)e->nslots, C = (size_t)e->cap;
        if (e->hdr.ensure(sizeof(SlotHdr) * S) || e->pts.ensure(48 * S * C) || e->err.ensure(32 * S * C) ||
            e->state.ensure(S * C) || e->chi2.ensure(16 * S * C) || e->Sout.ensure(64 * S) || e->nin.ensure(4 * S) ||
            e->iters.ensure(8 * S))
            return ORBX_EDEVICE;
        e->allocated = true;
    }
    return ORBX_OK;
}

// every check of a problem that needs no device
static int validate(const orbo_problem *p) {
    if (!p || p->n < 0 || p->n > kMaxPairs) return ORBX_EINVAL;
    if (p->n > 0 && (!p->X1c || !p->X2c || !p->obs1 || !p->obs2 || !p->inv_sigma2_1 || !p->inv_sigma2_2)) return ORBX_EINVAL;
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(p->q[k])) return ORBX_EINVAL;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(p->t[k])) return ORBX_EINVAL;
    if (!std::isfinite(p->s) || !(p->s > 0)) return ORBX_EINVAL;
    return ORBX_OK;
}

extern "C" {

int orbo_create(orbo_engine **out) {
    if (!out) return ORBX_EINVAL;
    *out = new orbo_engine();
    return ORBX_OK;
}

void orbo_destroy(orbo_engine *e) {
    if (!e) return;
    if (e->dev_ready) {
        (void)hipSetDevice(e->device);
        if (e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
        if (e->done) { (void)hipEventSynchronize(e->done); (void)hipEventDestroy(e->done); }
        DevBuf *bufs[] = {&e->hdr, &e->pts, &e->err, &e->state, &e->chi2, &e->Sout, &e->nin, &e->iters};
        for (DevBuf *b : bufs) b->release();
    }
    delete e;
}

int orbo_reserve(orbo_engine *e, int n_slots, int cap_pairs) {
    if (!e || n_slots <= 0 || n_slots > 65535 || cap_pairs < 0 || cap_pairs > kMaxPairs) return ORBX_EINVAL;
    e->nslots = n_slots;
    e->cap = std::max(cap_pairs, 1);
    e->n.assign(n_slots, -1);
    e->allocated = false;   // sized by the next call that reaches the device
    return ORBX_OK;
}

int orbo_stage(orbo_engine *e, int slot, const orbo_problem *p) {
    if (!e || slot < 0 || slot >= e->nslots) return ORBX_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    if (p->n > e->cap) return ORBX_ECAP;
    rc = ensure_device(e);
    if (rc) return rc;
    SlotHdr h{};
    h.n = p->n;
    h.fix_scale = p->fix_scale ? 1 : 0;
    h.th2 = p->th2;
    h.delta = (double)sqrtf(p->th2);
    for (int k = 0; k < 4; k++) {
        h.K1[k] = p->K1[k];
        h.K2[k] = p->K2[k];
        h.S.q[k] = p->q[k];
    }
    for (int k = 0; k < 3; k++) h.S.t[k] = p->t[k];
    h.S.s = p->s;
    e->tpts.resize((size_t)std::max(p->n, 1) * 3);
    for (int i = 0; i < p->n; i++) {
        const float *a = p->X1c + 3 * i, *b = p->X2c + 3 * i;
        e->tpts[3 * (size_t)i] = make_float4(a[0], a[1], a[2], p->inv_sigma2_1[i]);
        e->tpts[3 * (size_t)i + 1] = make_float4(b[0], b[1], b[2], p->inv_sigma2_2[i]);
        e->tpts[3 * (size_t)i + 2] = make_float4(p->obs1[2 * i], p->obs1[2 * i + 1], p->obs2[2 * i], p->obs2[2 * i + 1]);
    }
    const size_t s = (size_t)slot;
    hipStream_t st = e->stream;
    SO_CHK(order_after_done(e, st));
    SO_CHK(hipMemcpyAsync((char *)e->hdr.p + sizeof(SlotHdr) * s, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (p->n)
        SO_CHK(hipMemcpyAsync((char *)e->pts.p + 48 * s * (size_t)e->cap, e->tpts.data(), 48 * (size_t)p->n,
                              hipMemcpyHostToDevice, st));
    SO_CHK(hipStreamSynchronize(st));   // the staging vector is reused by the next slot
    e->n[slot] = p->n;
    return ORBX_OK;
}

int orbo_run_batch(orbo_engine *e, int n_slots, void *stream) {
    if (!e || n_slots <= 0 || n_slots > e->nslots) return ORBX_EINVAL;
    for (int s = 0; s < n_slots; s++)
        if (e->n[s] < 0) return ORBX_ESTATE;   // a slot that was never staged
    if (!e->dev_ready || !e->allocated) return ORBX_ESTATE;
    SO_CHK(hipSetDevice(e->device));
    Slots P;
    P.hdr = e->hdr.as<SlotHdr>(); P.pts = e->pts.as<float4>(); P.err = e->err.as<double>();
    P.state = e->state.as<uint8_t>(); P.chi2 = e->chi2.as<double>(); P.Sout = e->Sout.as<double>();
    P.nin = e->nin.as<int>(); P.iters = e->iters.as<int>(); P.cap = e->cap;
    const hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    SO_CHK(order_after_done(e, st));
    sim3_opt_kernel<<<n_slots, kThreads, 0, st>>>(P);
    SO_CHK(hipGetLastError());
    SO_CHK(mark_done(e, st));
    return ORBX_OK;
}

int orbo_fetch(orbo_engine *e, int slot, orbo_result *r) {
    if (!e || !r || slot < 0 || slot >= e->nslots) return ORBX_EINVAL;
    if (e->n[slot] > 0 && !r->state) return ORBX_EINVAL;
    if (!e->dev_ready || !e->allocated || e->n[slot] < 0) return ORBX_ESTATE;
    SO_CHK(hipSetDevice(e->device));
    const size_t s = (size_t)slot, C = (size_t)e->cap, n = (size_t)e->n[slot];
    double S[8];
    HostCopy hc(e->stream, e->done);
    hc.d2h(S, (char *)e->Sout.p + 64 * s, 64);
    hc.d2h(&r->n_inliers, (char *)e->nin.p + 4 * s, 4);
    hc.d2h(r->iterations, (char *)e->iters.p + 8 * s, 8);
    hc.d2h(r->state, (char *)e->state.p + s * C, n);
    hc.d2h(r->chi2, (char *)e->chi2.p + 16 * s * C, 16 * n);
    const int rc = hc.finish();
    if (rc) return rc;
    std::memcpy(r->q, S, 32);
    std::memcpy(r->t, S + 4, 24);
    r->s = S[7];
    return ORBX_OK;
}

int orbo_optimize_sim3(orbo_engine *e, const orbo_problem *p, orbo_result *r) {
    if (!e || !r) return ORBX_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    if (p->n > 0 && !r->state) return ORBX_EINVAL;
    if (e->nslots < 1 || e->cap < p->n) {
        rc = orbo_reserve(e, std::max(1, e->nslots), std::max(e->cap, p->n));
        if (rc) return rc;
    }
    rc = orbo_stage(e, 0, p);
    if (!rc) rc = orbo_run_batch(e, 1, nullptr);
    if (!rc) rc = orbo_fetch(e, 0, r);
    return rc;
}

}  // extern "C"
