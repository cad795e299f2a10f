// MI355X-native Sim3Solver hypothesis evaluation: the RANSAC body of LoopClosing::ComputeSim3
// (Sim3Solver::ComputeSim3 + CheckInliers, Sim3Solver.cc:330-488) for every hypothesis of every
// staged loop candidate in one launch.
//
// The hypotheses of a RANSAC run are independent; only "stop at the first iteration whose inlier
// count beats mRansacMinInliers" (Sim3Solver.cc:270-288) is sequential, and that is a scan over
// <= 300 integers the caller replays on the host. One wavefront owns one (slot, hypothesis): every
// lane repeats the closed-form Horn solve on the 3 sampled pairs (wave-uniform, no cross-lane
// traffic), then lane l tests correspondences l, l + 64, ... by the two-way reprojection of
// Project (:515-539) and the wave writes its inlier mask as ballot words.
//
// Precision follows the reference statement by statement (-ffp-contract=off): float centroids,
// M and N, a float Jacobi eigen-solve of the 4x4 N with cv::eigen's rotation formulas, double
// atan2 / Rodrigues rounded to a float R, double scale sums, float projections, Mat::dot in
// double rounded to float. cv::eigen visits pivots by magnitude, which needs run-time indices
// into the matrix; here the sweep is cyclic so every index is static and the kernel runs in
// registers (DESIGN.md "Sim3Solver numerics" states the agreement band this is tested to).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orb_device.h"
#include "orb_engine.h"
#include "orbslam2_amd.h"

using namespace orbamd;

#define S3_CHK(x)                                                                   \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "orbslam2_amd sim3: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return ORBX_EDEVICE;                                                    \
        }                                                                           \
    } while (0)

namespace orbs3 {

constexpr int kMaxN = 1 << 20;
constexpr int kWaves = 4;          // hypotheses per workgroup
constexpr int kMaxSweeps = 15;     // cyclic Jacobi sweeps (6 rotations each); 4x4 converges in 4-6

struct SlotHdr {
    int n, n_hyp, fix_scale, pad;
    float K1[4], K2[4];
};

struct Slots {
    const SlotHdr *hdr;
    const float4 *pts;          // [S][cap_n][3]: (X1c, P1im1.x) (X2c, P2im2.x) (P1im1.y, P2im2.y, maxErr1, maxErr2)
    const int *trip;            // [S][cap_hyp][3]
    int *n_inl;                 // [S][cap_hyp]
    unsigned long long *bits;   // [S][cap_hyp][words]
    float *R, *t, *s;           // [S][cap_hyp][9] / [3] / [1]
    int cap_n, cap_hyp, words;
};

__device__ __forceinline__ float cv_hypotf(float a, float b) {   // OpenCV's hypot(_Tp, _Tp), lapack.cpp
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) {
        b = b / a;
        return a * sqrtf(1 + b * b);
    }
    if (b > 0) {
        a = a / b;
        return b * sqrtf(1 + a * a);
    }
    return 0;
}

__device__ __forceinline__ void rot(float &v0, float &v1, float c, float s) {
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s;
    v1 = a0 * s + b0 * c;
}

// One Jacobi rotation of cv::eigen's JacobiImpl_<float> on the pivot (K, L), K < L: the upper
// triangle of A, the diagonal in W, eigenvectors in the rows of V. All indices are template
// constants. Returns false where the pivot is already <= FLT_EPSILON (a NaN pivot rotates).
template <int K, int L>
__device__ __forceinline__ bool jacobi_rotate(float (&A)[4][4], float (&W)[4], float (&V)[4][4]) {
    const float p = A[K][L];
    if (fabsf(p) <= FLT_EPSILON) return false;
    const float y = (W[L] - W[K]) * 0.5f;
    float t = fabsf(y) + cv_hypotf(p, y);
    float s = cv_hypotf(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) {
        s = -s;
        t = -t;
    }
    A[K][L] = 0;
    W[K] = W[K] - t;
    W[L] = W[L] + t;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < K) rot(A[i][K], A[i][L], c, s);
        if (i > K && i < L) rot(A[K][i], A[i][L], c, s);
        if (i > L) rot(A[K][i], A[L][i], c, s);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) rot(V[K][i], V[L][i], c, s);
    return true;
}

// Eigenvector of the largest eigenvalue of the symmetric 4x4 N (evec.row(0) of cv::eigen, which
// sorts descending with a strict compare: the first maximum stays in front).
__device__ __forceinline__ void eigen4_top(float (&A)[4][4], float q[4]) {
    float W[4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        W[i] = A[i][i];
#pragma unroll
        for (int k = 0; k < 4; k++) V[i][k] = i == k ? 1.0f : 0.0f;
    }
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        bool any = false;
        any |= jacobi_rotate<0, 1>(A, W, V);
        any |= jacobi_rotate<0, 2>(A, W, V);
        any |= jacobi_rotate<0, 3>(A, W, V);
        any |= jacobi_rotate<1, 2>(A, W, V);
        any |= jacobi_rotate<1, 3>(A, W, V);
        any |= jacobi_rotate<2, 3>(A, W, V);
        if (!any) break;
    }
    float bw = W[0];
    q[0] = V[0][0]; q[1] = V[0][1]; q[2] = V[0][2]; q[3] = V[0][3];
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const bool gt = bw < W[i];
        bw = gt ? W[i] : bw;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = gt ? V[i][k] : q[k];
    }
}

__device__ __forceinline__ float dot3f(const float *a, float x, float y, float z) {   // one row of a float gemm
    float s = a[0] * x;
    s = s + a[1] * y;
    s = s + a[2] * z;
    return s;
}

// Project (Sim3Solver.cc:515-539): R * X + t, invz = 1 / z with no sign test, K applied in float
__device__ __forceinline__ void project(const float T[12], const float K[4], float x, float y, float z, float &u, float &v) {
    const float px = dot3f(T, x, y, z) + T[9];
    const float py = dot3f(T + 3, x, y, z) + T[10];
    const float pz = dot3f(T + 6, x, y, z) + T[11];
    const float invz = 1 / pz;
    u = K[0] * (px * invz) + K[2];
    v = K[1] * (py * invz) + K[3];
}

__device__ __forceinline__ float sqdist(float ax, float ay, float bx, float by) {   // dist.dot(dist): Mat::dot -> float
    const float dx = ax - bx, dy = ay - by;
    double r = 0;
    r += (double)dx * dx;
    r += (double)dy * dy;
    return (float)r;
}

__global__ __launch_bounds__(64 * kWaves) void sim3_hypotheses_kernel(Slots S) {
    const int slot = blockIdx.y;
    const int hyp = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const SlotHdr &H = S.hdr[slot];
    const int n = H.n;
    if (hyp >= H.n_hyp) return;   // wave-uniform
    const float4 *pts = S.pts + (size_t)slot * S.cap_n * 3;
    const size_t ho = (size_t)slot * S.cap_hyp + hyp;

    // ---- ComputeSim3 (Sim3Solver.cc:330-452), redundantly in every lane ----
    float P1[3][3], P2[3][3];   // [coordinate][sample], as P3Dc1i / P3Dc2i
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int idx = S.trip[ho * 3 + j];   // checked against [0, n) by the host
        const float4 a = pts[(size_t)idx * 3], b = pts[(size_t)idx * 3 + 1];
        P1[0][j] = a.x; P1[1][j] = a.y; P1[2][j] = a.z;
        P2[0][j] = b.x; P2[1][j] = b.y; P2[2][j] = b.z;
    }
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
    const float third = (float)(1.0 / 3);   // C / P.cols: a float scale by 1 / 3
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) * third;
        O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) * third;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Pr1[r][j] = P1[r][j] - O1[r];
            Pr2[r][j] = P2[r][j] - O2[r];
        }
    }
    float M[3][3];   // Pr2 * Pr1.t()
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r][c] = dot3f(Pr2[r], Pr1[c][0], Pr1[c][1], Pr1[c][2]);
    float N[4][4];   // the float sums of :356-365, upper triangle + diagonal
    N[0][0] = M[0][0] + M[1][1] + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = M[0][0] - M[1][1] - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = -M[0][0] + M[1][1] - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = -M[0][0] - M[1][1] + M[2][2];
    N[1][0] = N[2][0] = N[3][0] = N[2][1] = N[3][1] = N[3][2] = 0;   // never read
    float q[4];
    eigen4_top(N, q);
    // ang = atan2(norm(vec), q0); vec = 2 * ang * vec / norm(vec) (:386-389)
    double nv = 0;
    nv += (double)q[1] * q[1];
    nv += (double)q[2] * q[2];
    nv += (double)q[3] * q[3];
    nv = sqrt(nv);
    const double ang = atan2(nv, (double)q[0]);
    const float alpha = (float)(2 * ang / nv);
    const double rx0 = (double)(q[1] * alpha), ry0 = (double)(q[2] * alpha), rz0 = (double)(q[3] * alpha);
    // cv::Rodrigues(vec, R) in double, rounded to the float R
    const double theta = sqrt(rx0 * rx0 + ry0 * ry0 + rz0 * rz0);
    float R[9];
    if (theta < DBL_EPSILON) {
        R[0] = R[4] = R[8] = 1.0f;
        R[1] = R[2] = R[3] = R[5] = R[6] = R[7] = 0.0f;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1. - c, it = 1 / theta;
        const double rx = rx0 * it, ry = ry0 * it, rz = rz0 * it;
        R[0] = (float)(c + c1 * (rx * rx));
        R[1] = (float)(c1 * (rx * ry) + s * -rz);
        R[2] = (float)(c1 * (rx * rz) + s * ry);
        R[3] = (float)(c1 * (rx * ry) + s * rz);
        R[4] = (float)(c + c1 * (ry * ry));
        R[5] = (float)(c1 * (ry * rz) + s * -rx);
        R[6] = (float)(c1 * (rx * rz) + s * -ry);
        R[7] = (float)(c1 * (ry * rz) + s * rx);
        R[8] = (float)(c + c1 * (rz * rz));
    }
    float sc = 1.0f;
    if (!H.fix_scale) {   // nom = Pr1.dot(P3), den = sum(P3^2), both accumulated in double (:405-422)
        double nom = 0, den = 0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float p3 = dot3f(R + 3 * r, Pr2[0][j], Pr2[1][j], Pr2[2][j]);
                nom += (double)Pr1[r][j] * p3;
                den += (double)(p3 * p3);
            }
        sc = (float)(nom / den);
    }
    float T12[12], T21[12];   // [R(9) | t(3)] of mT12i / mT21i (:435-451)
    const float sinv = (float)(1.0 / (double)sc);
    float t12[3];
#pragma unroll
    for (int r = 0; r < 3; r++) t12[r] = O1[r] - sc * dot3f(R + 3 * r, O2[0], O2[1], O2[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            T12[3 * r + c] = sc * R[3 * r + c];
            T21[3 * r + c] = sinv * R[3 * c + r];
        }
        T12[9 + r] = t12[r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) T21[9 + r] = -dot3f(T21 + 3 * r, t12[0], t12[1], t12[2]);

    // ---- CheckInliers (:458-488): correspondences lane, lane + 64, ... ----
    float K1[4], K2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        K1[k] = H.K1[k];
        K2[k] = H.K2[k];
    }
    unsigned long long *bits = S.bits + ho * S.words;
    int count = 0;
    for (int w = 0; w * 64 < n; w++) {
        const int i = w * 64 + lane;
        bool in = false;
        if (i < n) {
            const float4 a = pts[(size_t)i * 3], b = pts[(size_t)i * 3 + 1], c = pts[(size_t)i * 3 + 2];
            float u21, v21, u12, v12;
            project(T12, K1, b.x, b.y, b.z, u21, v21);   // vP2im1
            project(T21, K2, a.x, a.y, a.z, u12, v12);   // vP1im2
            const float err1 = sqdist(a.w, c.x, u21, v21);
            const float err2 = sqdist(u12, v12, b.w, c.y);
            in = err1 < c.z && err2 < c.w;   // NaN / Inf compare false
        }
        const unsigned long long bal = __ballot(in);
        count += __popcll(bal);
        if (lane == 0) bits[w] = bal;
    }
    if (lane == 0) {
        S.n_inl[ho] = count;
        float *Ro = S.R + ho * 9, *to = S.t + ho * 3;
#pragma unroll
        for (int k = 0; k < 9; k++) Ro[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) to[k] = t12[k];
        S.s[ho] = sc;
    }
}

}  // namespace orbs3

using namespace orbs3;

struct orbs_engine {
    bool dev_ready = false;   // the device is first touched by a call whose arguments passed every check
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    int nslots = 0, cap_n = 0, cap_hyp = 0, words = 0;
    bool allocated = false;
    std::vector<SlotHdr> h;
    DevBuf hdr, pts, trip, n_inl, bits, R, t, s;
    std::vector<float4> tpts;
};

static int ensure_device(orbs_engine *e) {
    if (!e->dev_ready) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return ORBX_EDEVICE;
        if (hipGetDevice(&e->device) != hipSuccess) return ORBX_EDEVICE;
        if (!e->stream && hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return ORBX_EDEVICE;
        if (!e->done && !(e->done = make_done_event())) return ORBX_EDEVICE;
        e->dev_ready = true;
    }
    S3_CHK(hipSetDevice(e->device));
    if (!e->allocated) {
        const size_t S = (size_t)e->nslots, C = (size_t)e->cap_n, Hy = (size_t)e->cap_hyp, W = (size_t)e->words;
        if (e->hdr.ensure(sizeof(SlotHdr) * S) || e->pts.ensure(48 * S * C) || e->trip.ensure(12 * S * Hy) ||
            e->n_inl.ensure(4 * S * Hy) || e->bits.ensure(8 * S * Hy * W) || e->R.ensure(36 * S * Hy) ||
            e->t.ensure(12 * S * Hy) || e->s.ensure(4 * S * Hy))
            return ORBX_EDEVICE;
        e->allocated = true;
    }
    return ORBX_OK;
}

static Slots make_slots(orbs_engine *e) {
    Slots S;
    S.hdr = e->hdr.as<SlotHdr>();
    S.pts = e->pts.as<float4>();
    S.trip = e->trip.as<int>();
    S.n_inl = e->n_inl.as<int>();
    S.bits = e->bits.as<unsigned long long>();
    S.R = e->R.as<float>();
    S.t = e->t.as<float>();
    S.s = e->s.as<float>();
    S.cap_n = e->cap_n;
    S.cap_hyp = e->cap_hyp;
    S.words = e->words;
    return S;
}

// every check of a problem that needs no device: the kernel indexes with n, n_hyp and the triplets
static int validate(const orbs_problem *p, int cap_n, int cap_hyp) {
    if (!p || !p->X1c || !p->X2c || !p->max_err1 || !p->max_err2 || !p->triplets) return ORBX_EINVAL;
    if (p->n < 3 || p->n > cap_n || p->n_hyp < 1 || p->n_hyp > ORBS_MAX_HYP || p->n_hyp > cap_hyp) return ORBX_EINVAL;
    for (int h = 0; h < p->n_hyp; h++) {
        const int32_t a = p->triplets[3 * h], b = p->triplets[3 * h + 1], c = p->triplets[3 * h + 2];
        if (a < 0 || a >= p->n || b < 0 || b >= p->n || c < 0 || c >= p->n) return ORBX_EINVAL;
        if (a == b || a == c || b == c) return ORBX_EINVAL;
    }
    return ORBX_OK;
}

static bool result_ok(const orbs_result *r) {
    return r && r->n_inliers && r->inlier_bits && r->R12 && r->t12 && r->s12;
}

extern "C" {

int orbs_create(orbs_engine **out) {
    if (!out) return ORBX_EINVAL;
    *out = new orbs_engine();
    return ORBX_OK;
}

void orbs_destroy(orbs_engine *e) {
    if (!e) return;
    if (e->dev_ready) {
        (void)hipSetDevice(e->device);
        if (e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
        if (e->done) { (void)hipEventSynchronize(e->done); (void)hipEventDestroy(e->done); }
        DevBuf *bufs[] = {&e->hdr, &e->pts, &e->trip, &e->n_inl, &e->bits, &e->R, &e->t, &e->s};
        for (DevBuf *b : bufs) b->release();
    }
    delete e;
}

int orbs_reserve(orbs_engine *e, int n_slots, int cap_n, int cap_hyp) {
    if (!e || n_slots <= 0 || n_slots > 65535 || cap_n < 3 || cap_n > kMaxN || cap_hyp < 1 || cap_hyp > ORBS_MAX_HYP)
        return ORBX_EINVAL;
    e->nslots = n_slots;
    e->cap_n = cap_n;
    e->cap_hyp = cap_hyp;
    e->words = (cap_n + 63) / 64;
    e->h.assign(n_slots, SlotHdr{});
    e->allocated = false;   // sized by the next call that reaches the device
    return ORBX_OK;
}

int orbs_stage(orbs_engine *e, int slot, const orbs_problem *p) {
    if (!e || slot < 0 || slot >= e->nslots) return ORBX_EINVAL;
    int rc = validate(p, e->cap_n, e->cap_hyp);
    if (rc) return rc;
    rc = ensure_device(e);
    if (rc) return rc;
    SlotHdr &h = e->h[slot];
    h = SlotHdr{};
    h.n = p->n;
    h.n_hyp = p->n_hyp;
    h.fix_scale = p->fix_scale ? 1 : 0;
    std::memcpy(h.K1, p->K1, sizeof h.K1);
    std::memcpy(h.K2, p->K2, sizeof h.K2);
    e->tpts.resize((size_t)p->n * 3);
    for (int i = 0; i < p->n; i++) {   // FromCameraToImage (Sim3Solver.cc:548-567)
        const float *a = p->X1c + 3 * i, *b = p->X2c + 3 * i;
        const float iz1 = 1 / a[2], iz2 = 1 / b[2];
        const float u1 = p->K1[0] * (a[0] * iz1) + p->K1[2], v1 = p->K1[1] * (a[1] * iz1) + p->K1[3];
        const float u2 = p->K2[0] * (b[0] * iz2) + p->K2[2], v2 = p->K2[1] * (b[1] * iz2) + p->K2[3];
        e->tpts[3 * (size_t)i] = make_float4(a[0], a[1], a[2], u1);
        e->tpts[3 * (size_t)i + 1] = make_float4(b[0], b[1], b[2], u2);
        e->tpts[3 * (size_t)i + 2] = make_float4(v1, v2, p->max_err1[i], p->max_err2[i]);
    }
    const size_t s = (size_t)slot;
    hipStream_t st = e->stream;
    S3_CHK(order_after_done(e, st));
    S3_CHK(hipMemcpyAsync((char *)e->hdr.p + sizeof(SlotHdr) * s, &h, sizeof h, hipMemcpyHostToDevice, st));
    S3_CHK(hipMemcpyAsync((char *)e->pts.p + 48 * s * (size_t)e->cap_n, e->tpts.data(), 48 * (size_t)p->n,
                          hipMemcpyHostToDevice, st));
    S3_CHK(hipMemcpyAsync((char *)e->trip.p + 12 * s * (size_t)e->cap_hyp, p->triplets, 12 * (size_t)p->n_hyp,
                          hipMemcpyHostToDevice, st));
    S3_CHK(hipStreamSynchronize(st));   // the staging vector is reused by the next slot
    return ORBX_OK;
}

int orbs_run_batch(orbs_engine *e, int n_slots, void *stream) {
    if (!e || n_slots <= 0 || n_slots > e->nslots) return ORBX_EINVAL;
    int maxh = 0;
    for (int s = 0; s < n_slots; s++) {
        if (e->h[s].n_hyp < 1) return ORBX_ESTATE;   // a slot that was never staged
        maxh = std::max(maxh, e->h[s].n_hyp);
    }
    if (!e->dev_ready || !e->allocated) return ORBX_ESTATE;
    S3_CHK(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    S3_CHK(order_after_done(e, st));
    sim3_hypotheses_kernel<<<dim3((maxh + kWaves - 1) / kWaves, n_slots), 64 * kWaves, 0, st>>>(make_slots(e));
    S3_CHK(hipGetLastError());
    S3_CHK(mark_done(e, st));
    return ORBX_OK;
}

int orbs_fetch(orbs_engine *e, int slot, orbs_result *r) {
    if (!e || slot < 0 || slot >= e->nslots || !result_ok(r)) return ORBX_EINVAL;
    if (!e->dev_ready || !e->allocated || e->h[slot].n_hyp < 1) return ORBX_ESTATE;
    S3_CHK(hipSetDevice(e->device));
    const size_t s = (size_t)slot, Hy = (size_t)e->cap_hyp, nh = (size_t)e->h[slot].n_hyp;
    const size_t w = ((size_t)e->h[slot].n + 63) / 64;
    HostCopy hc(e->stream, e->done);
    hc.d2h(r->n_inliers, (char *)e->n_inl.p + 4 * s * Hy, 4 * nh);
    hc.d2h(r->R12, (char *)e->R.p + 36 * s * Hy, 36 * nh);
    hc.d2h(r->t12, (char *)e->t.p + 12 * s * Hy, 12 * nh);
    hc.d2h(r->s12, (char *)e->s.p + 4 * s * Hy, 4 * nh);
    if (hc.err == hipSuccess)   // rows of (n + 63) / 64 words out of rows of `words`
        hc.err = hipMemcpy2DAsync(r->inlier_bits, 8 * w, (char *)e->bits.p + 8 * s * Hy * (size_t)e->words,
                                  8 * (size_t)e->words, 8 * w, nh, hipMemcpyDeviceToHost, e->stream);
    return hc.finish();
}

int orbs_evaluate(orbs_engine *e, const orbs_problem *p, orbs_result *r) {
    if (!e || !result_ok(r)) return ORBX_EINVAL;
    int rc = validate(p, kMaxN, ORBS_MAX_HYP);
    if (rc) return rc;
    if (e->nslots < 1 || e->cap_n < p->n || e->cap_hyp < p->n_hyp) {
        rc = orbs_reserve(e, std::max(1, e->nslots), std::max(e->cap_n, p->n), std::max(e->cap_hyp, p->n_hyp));
        if (rc) return rc;
    }
    rc = orbs_stage(e, 0, p);
    if (!rc) rc = orbs_run_batch(e, 1, nullptr);
    if (!rc) rc = orbs_fetch(e, 0, r);
    return rc;
}

}  // extern "C"
