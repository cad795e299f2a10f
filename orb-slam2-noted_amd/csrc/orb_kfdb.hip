// MI355X-native KeyFrameDatabase: add / erase / clear, DetectLoopCandidates and
// DetectRelocalizationCandidates (KeyFrameDatabase.cc:57-418) and the mpVoc->score scan of
// LoopClosing::DetectLoop (LoopClosing.cc:163-184), on BowVectors that stay in HBM.
//
// The reference walks an inverted file; its outputs depend on three things only, and a scan over all
// keyframes gives the same three: the number of words a keyframe shares with the query (mnLoopWords /
// mnRelocWords), the L1 score, and the order of lKFsSharingWords, which is (first common word id, position
// in that word's inverted list) = (first common word id, add sequence number).
//   kfdb_score_kernel    one wavefront per (query, keyframe), 16 to a workgroup sharing the query BowVector in
//                        LDS: lanes binary-search the keyframe's words, two chunks of 64 at a time, a ballot
//                        gives the shared-word count and the first common word,
//                        and the matched terms are added in word order (L1Scoring::score's double sum is one
//                        serial chain: no tree reduction), then -score / 2.0 rounded to float
//   kfdb_select_kernel   one workgroup per query: maxCommonWords, minCommonWords = (int)(max * 0.8f), the
//                        keyframes of lScoreAndMatch ranked by (first common word, sequence)
//   kfdb_groups_kernel   one workgroup per query: the covisibility groups, bestAccScore, minScoreToRetain =
//                        0.75f * bestAccScore, first occurrence of each best keyframe. A relocalisation query
//                        reads the mRelocScore earlier queries left; inside a run that is the si of the latest
//                        earlier relocalisation query the neighbour passed in, looked up, so the queries of a
//                        run do not wait for each other
//   kfdb_state_kernel    leaves mRelocScore as the run's last such query set it
// Every query is a fresh query id: the reference's behaviour for a repeated mnId, or for id 0 against
// keyframes whose mnLoopQuery / mnRelocQuery are still 0, is not reproduced. mRelocScore, which the
// reference reads uninitialised from a keyframe that never passed the word threshold, is pinned to 0.0f.
// BowVector values must be finite (the strict > chains of the reference are restated as maxima).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "orb_device.h"
#include "orb_engine.h"
#include "orbslam2_amd.h"

using namespace orbamd;

#define KD_CHK(x)                                                                   \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "orbslam2_amd kfdb: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return ORBX_EDEVICE;                                                    \
        }                                                                           \
    } while (0)

namespace orbkfdb {

constexpr int kWaves = 16;       // wavefronts = keyframes per workgroup of the score kernel, sharing one LDS copy of the query
constexpr int kCov = ORBD_MAX_COVISIBLES;
constexpr int kQW = ORBD_MAX_WORDS;   // words per staged query row
constexpr int kSelThreads = 1024;

struct KfMeta {
    long long off;   // first word in the pool
    long long id;    // KeyFrame::mnId
    unsigned seq;    // add sequence number
    int len;         // BowVector length, -1 = free slot
};

struct QHdr {
    int kind;
    float min_score;
};

struct ScoreArgs {
    const uint32_t *pool_w;
    const double *pool_v;
    const KfMeta *meta;
    int n_slots;              // slots in use (free ones included)
    const uint32_t *qw;       // [rows][kQW]
    const double *qv;
    const int *qn;            // [rows]
    int q_cap;                // an upper bound of the launch's query lengths: the LDS copy holds this many words
    int row0;
    const int *slot_list;     // orbd_scores: the keyframes to score, or NULL = every slot
    int n_list;
    int *cnt;                 // [rows][row_stride] shared words
    uint32_t *fw;             // first common word
    float *si;                // (float)L1Scoring::score
    int row_stride;
};

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// One chunk of 64 keyframe words after the search: the shared-word count, the first common word, and the matched
// terms added to the score in lane (= ascending word) order.
__device__ __forceinline__ void take_chunk(bool hit, uint32_t w, double term, int &count, uint32_t &first, double &score) {
    unsigned long long bal = __ballot(hit);
    if (!bal) return;
    if (count == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)w, __ffsll((long long)bal) - 1);
    count += __popcll(bal);
    while (bal) {   // score += term: L1Scoring::score's serial double sum
        const int l = __ffsll((long long)bal) - 1;
        bal &= bal - 1;
        score = score + readlane_f64(term, l);
    }
}

__global__ __launch_bounds__(64 * kWaves) void kfdb_score_kernel(ScoreArgs A) {
    extern __shared__ double q_v[];                       // [q_cap] values, then [q_cap] words
    uint32_t *q_w = (uint32_t *)(q_v + A.q_cap);
    const int row = A.row0 + blockIdx.y;
    const int qn = max(0, min(A.qn[row], A.q_cap));
    for (int i = threadIdx.x; i < qn; i += 64 * kWaves) {
        q_w[i] = A.qw[(size_t)row * kQW + i];
        q_v[i] = A.qv[(size_t)row * kQW + i];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int items = A.slot_list ? A.n_list : A.n_slots;
    const size_t orow = A.slot_list ? 0 : (size_t)row * A.row_stride;
    const int top = qn > 0 ? 1 << (31 - __clz(qn)) : 0;   // largest power of two <= qn
    const int item = blockIdx.x * kWaves + wave;
    if (item >= items) return;   // wave-uniform, after the only barrier
    const int slot = A.slot_list ? A.slot_list[item] : item;   // checked against [0, n_slots) by the host
    const KfMeta m = A.meta[slot];
    const uint32_t *pw = A.pool_w + m.off;
    const double *pv = A.pool_v + m.off;
    int count = 0;
    uint32_t first = 0xffffffffu;
    double score = 0;
    for (int base = 0; base < m.len; base += 128) {   // two chunks per turn: their searches overlap
        const int i0 = base + lane, i1 = i0 + 64;
        const bool a0 = i0 < m.len, a1 = i1 < m.len;
        const uint32_t w0 = a0 ? pw[i0] : 0u, w1 = a1 ? pw[i1] : 0u;
        const double x0 = a0 ? pv[i0] : 0.0, x1 = a1 ? pv[i1] : 0.0;
        int l0 = 0, l1 = 0;   // query words below w0 / w1: a lower_bound in log2(qn) uniform steps
        for (int s = top; s > 0; s >>= 1) {
            const int m0 = l0 + s, m1 = l1 + s;
            if (m0 <= qn && q_w[m0 - 1] < w0) l0 = m0;
            if (m1 <= qn && q_w[m1 - 1] < w1) l1 = m1;
        }
        const bool h0 = a0 && l0 < qn && q_w[l0] == w0, h1 = a1 && l1 < qn && q_w[l1] == w1;
        double t0 = 0, t1 = 0;
        if (h0) { const double vi = q_v[l0]; t0 = (fabs(vi - x0) - fabs(vi)) - fabs(x0); }   // v1 = the query, v2 = the keyframe
        if (h1) { const double vi = q_v[l1]; t1 = (fabs(vi - x1) - fabs(vi)) - fabs(x1); }
        take_chunk(h0, w0, t0, count, first, score);
        take_chunk(h1, w1, t1, count, first, score);
    }
    if (lane == 0) {
        score = -score / 2.0;
        A.cnt[orow + item] = count;
        A.fw[orow + item] = first;
        A.si[orow + item] = (float)score;
    }
}

// One query's record going in (the header and the connected mask, one upload per run) and coming out (one
// download per run): rows of in_bytes / out_bytes, laid out for `stride` keyframe slots.
struct RowIn {
    const QHdr *qh;
    const uint8_t *excl;   // [stride] 1 = in the loop query's connected set
};
struct RowOut {
    int4 *hdr;             // n_scored, n_candidates, minCommonWords, maxCommonWords
    long long *sm_id;      // lScoreAndMatch in list order: keyframe id,
    long long *best_id;    //   pBestKF of its group,
    long long *cand;       // the candidates
    float *sm_si;          //   si,
    float *acc;            //   accScore of its group,
    int *sm_words;         //   shared words
};
__host__ __device__ inline size_t row_in_bytes(int stride) { return 8 + (((size_t)stride + 7) & ~(size_t)7); }
__host__ __device__ inline size_t row_out_bytes(int stride) { return (16 + 36 * (size_t)stride + 15) & ~(size_t)15; }
__host__ __device__ inline RowIn row_in(const void *base, int stride, int row) {
    const char *p = (const char *)base + row_in_bytes(stride) * row;
    return RowIn{(const QHdr *)p, (const uint8_t *)p + 8};
}
__host__ __device__ inline RowOut row_out(void *base, int stride, int row) {
    char *p = (char *)base + row_out_bytes(stride) * row;
    RowOut o;
    o.hdr = (int4 *)p;
    o.sm_id = (long long *)(p + 16);
    o.best_id = o.sm_id + stride;
    o.cand = o.best_id + stride;
    o.sm_si = (float *)(o.cand + stride);
    o.acc = o.sm_si + stride;
    o.sm_words = (int *)(o.acc + stride);
    return o;
}

struct SelArgs {
    const KfMeta *meta;
    int n_slots;
    const void *in;             // RowIn records, [rows]
    void *out;                  // RowOut records, [rows]
    const int *cnt;             // [rows][row_stride], as ScoreArgs
    const uint32_t *fw;
    const float *si;
    unsigned long long *tkey;   // [rows][row_stride] unordered (first word, sequence) keys
    int *tslot;
    int *sm_slot;               // slots of lScoreAndMatch in list order
    int *best;                  // slot of pBestKF
    int *flag;
    const int *covis;           // [n_slots][kCov] slot of the j-th best covisible, -1 = none / not in the database
    float *reloc_score;         // [n_slots] mRelocScore as the run found it
    int row_stride;
    int row0, n_rows;
};

__global__ __launch_bounds__(kSelThreads) void kfdb_select_kernel(SelArgs A) {
    __shared__ int s_max, s_n;
    const int row = A.row0 + blockIdx.x, tid = threadIdx.x;
    const size_t ro = (size_t)row * A.row_stride;
    const RowIn I = row_in(A.in, A.row_stride, row);
    const RowOut O = row_out(A.out, A.row_stride, row);
    const bool loop = I.qh->kind == ORBD_LOOP;
    const float min_score = I.qh->min_score;
    if (tid == 0) { s_max = 0; s_n = 0; }
    __syncthreads();
    int mx = 0;
    for (int s = tid; s < A.n_slots; s += kSelThreads)
        if (!(loop && I.excl[s])) mx = max(mx, A.cnt[ro + s]);
    if (mx) atomicMax(&s_max, mx);
    __syncthreads();
    const int maxc = s_max;
    const int minc = (int)((float)maxc * 0.8f);
    if (maxc == 0) {   // lKFsSharingWords.empty()
        if (tid == 0) *O.hdr = make_int4(0, 0, 0, 0);
        return;
    }
    for (int s = tid; s < A.n_slots; s += kSelThreads) {
        const bool pass = A.cnt[ro + s] > minc && !(loop && I.excl[s]);
        if (pass && (!loop || A.si[ro + s] >= min_score)) {
            const int p = atomicAdd(&s_n, 1);
            A.tkey[ro + p] = ((unsigned long long)A.fw[ro + s] << 32) | A.meta[s].seq;
            A.tslot[ro + p] = s;
        }
    }
    __syncthreads();
    const int P = s_n;
    for (int i = tid; i < P; i += kSelThreads) {   // keys are distinct (the sequence is): ranks are a permutation
        const unsigned long long key = A.tkey[ro + i];
        int r = 0;
        for (int j = 0; j < P; j++) r += A.tkey[ro + j] < key;
        const int s = A.tslot[ro + i];
        A.sm_slot[ro + r] = s;
        O.sm_id[r] = A.meta[s].id;
        O.sm_si[r] = A.si[ro + s];
        O.sm_words[r] = A.cnt[ro + s];
    }
    if (tid == 0) *O.hdr = make_int4(P, 0, minc, maxc);
}

// Did keyframe slot `s` pass the word threshold of relocalisation query `row` (and so get its mRelocScore there)?
__device__ __forceinline__ bool reloc_passed(const SelArgs &A, int row, int s) {
    if (row_in(A.in, A.row_stride, row).qh->kind != ORBD_RELOC) return false;
    const int minc = ((const int *)row_out(A.out, A.row_stride, row).hdr)[2];   // that word alone: .y is being written
    return A.cnt[(size_t)row * A.row_stride + s] > minc;   // no shared word: 0 > 0 fails
}

// One workgroup per query. mRelocScore as query `row` of the run sees it: the si of the latest relocalisation
// query up to and including this one in which the keyframe passed, else the value the run found -- what issuing
// the queries one after another leaves, without the queries waiting for each other.
__global__ __launch_bounds__(kSelThreads) void kfdb_groups_kernel(SelArgs A) {
    __shared__ float s_red[kSelThreads];
    __shared__ int s_cnt;
    const int row = A.row0 + blockIdx.x, tid = threadIdx.x;
    const size_t ro = (size_t)row * A.row_stride;
    const RowIn I = row_in(A.in, A.row_stride, row);
    const RowOut O = row_out(A.out, A.row_stride, row);
    const int4 h = *O.hdr;
    const int P = h.x, minc = h.z;
    if (P == 0) return;   // uniform: lScoreAndMatch.empty()
    const bool loop = I.qh->kind == ORBD_LOOP;
    if (tid == 0) s_cnt = 0;
    float top = loop ? I.qh->min_score : 0.0f;   // bestAccScore
    for (int i = tid; i < P; i += kSelThreads) {
        const int s = A.sm_slot[ro + i];
        float acc = O.sm_si[i], bs = acc;
        int bk = s;
        for (int c = 0; c < kCov; c++) {
            const int ns = A.covis[(size_t)s * kCov + c];
            if (ns < 0) continue;
            float sc;
            if (loop) {
                if (!(A.cnt[ro + ns] > minc) || I.excl[ns]) continue;
                sc = A.si[ro + ns];
            } else {
                if (A.cnt[ro + ns] <= 0) continue;   // mnRelocQuery != F->mnId
                sc = A.reloc_score[ns];
                for (int r = row; r >= A.row0; r--)
                    if (reloc_passed(A, r, ns)) { sc = A.si[(size_t)r * A.row_stride + ns]; break; }
            }
            acc = acc + sc;
            if (sc > bs) { bs = sc; bk = ns; }
        }
        O.acc[i] = acc;
        A.best[ro + i] = bk;
        O.best_id[i] = A.meta[bk].id;
        if (acc > top) top = acc;
    }
    s_red[tid] = top;
    __syncthreads();
    for (int off = kSelThreads / 2; off > 0; off >>= 1) {
        if (tid < off && s_red[tid + off] > s_red[tid]) s_red[tid] = s_red[tid + off];
        __syncthreads();
    }
    const float retain = 0.75f * s_red[0];   // minScoreToRetain
    for (int i = tid; i < P; i += kSelThreads) {
        bool keep = O.acc[i] > retain;
        const int b = A.best[ro + i];
        for (int j = 0; keep && j < i; j++) keep = !(O.acc[j] > retain && A.best[ro + j] == b);   // spAlreadyAddedKF
        A.flag[ro + i] = keep;
    }
    __syncthreads();
    for (int i = tid; i < P; i += kSelThreads) {
        if (!A.flag[ro + i]) continue;
        int pos = 0;
        for (int j = 0; j < i; j++) pos += A.flag[ro + j];
        O.cand[pos] = O.best_id[i];
        atomicAdd(&s_cnt, 1);
    }
    __syncthreads();
    if (tid == 0) O.hdr->y = s_cnt;
}

// After every query of the run: mRelocScore of a keyframe = the si of the last relocalisation query it passed in
__global__ __launch_bounds__(256) void kfdb_state_kernel(SelArgs A) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= A.n_slots) return;
    for (int r = A.row0 + A.n_rows - 1; r >= A.row0; r--)
        if (reloc_passed(A, r, s)) {
            A.reloc_score[s] = A.si[(size_t)r * A.row_stride + s];
            return;
        }
}

struct HostRes {   // one run's RowOut records, in page-locked host memory
    int rows = 0, stride = 0;
    PinnedBuf buf;
    int shape(int n, int st) {
        if (buf.ensure(row_out_bytes(st) * n)) return ORBX_EDEVICE;
        rows = n;
        stride = st;
        return ORBX_OK;
    }
};

struct StagedQuery {
    bool staged = false;
    int n_upper = 0;   // the BowVector's length, or the row capacity where only the device knows it
    int kind = 0;
    float min_score = 0;
    std::vector<long long> connected;
};

}  // namespace orbkfdb

using namespace orbkfdb;

struct orbd_db {
    std::mutex mu;   // the reference's mMutex
    int n_words = 0;
    bool dev_ready = false;   // the device is first touched by a call whose arguments passed every check
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;   // end of the last orbd_run_batch
    bool pending = false;        // that batch has not been waited for yet
    // keyframes
    std::unordered_map<long long, int> slot_of;
    std::vector<KfMeta> meta;                 // host mirror, [hi]
    std::vector<std::vector<long long>> cov;  // covisible ids per slot
    std::vector<int> free_slots;
    int hi = 0, slot_cap = 0;
    unsigned next_seq = 0;
    size_t pool_used = 0, pool_cap = 0, live_words = 0;
    bool cov_dirty = true;
    DevBuf pool_w, pool_v, d_meta, d_cov, d_reloc;
    // staged queries: rows [0, nq) and the single-call row nq
    int nq = 0;
    std::vector<StagedQuery> q;
    DevBuf qw, qv, qn, d_in, d_out;
    DevBuf cnt, fw, si, tkey, tslot, sm_slot, best, flag;
    int work_rows = 0, work_stride = 0;
    DevBuf sc_list, sc_cnt, sc_fw, sc_si;   // orbd_scores
    HostRes batch, single;
    PinnedBuf h_in;   // staging of a run's RowIn records: untouched until the run is done
};

namespace {

int ensure_device(orbd_db *d) {
    if (!d->dev_ready) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return ORBX_EDEVICE;
        if (hipGetDevice(&d->device) != hipSuccess) return ORBX_EDEVICE;
        if (!d->stream && hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return ORBX_EDEVICE;
        if (!d->done && !(d->done = make_done_event())) return ORBX_EDEVICE;
        d->dev_ready = true;
    }
    KD_CHK(hipSetDevice(d->device));
    return ORBX_OK;
}

// The one host synchronisation of a batch: whichever entry comes after orbd_run_batch waits for it here, so
// nothing that run reads or writes (the database, the staging records, the result block) changes under it.
int settle(orbd_db *d) {
    if (!d->pending) return ORBX_OK;
    KD_CHK(hipSetDevice(d->device));
    KD_CHK(hipEventSynchronize(d->done));
    d->pending = false;
    return ORBX_OK;
}

// query rows live for nq + 1 rows; (re)sized when orbd_reserve changed nq
int ensure_query_rows(orbd_db *d) {
    const size_t R = (size_t)d->nq + 1;
    if (d->qw.bytes >= 4 * R * kQW && d->qw.p) return ORBX_OK;
    if (d->qw.ensure(4 * R * kQW) || d->qv.ensure(8 * R * kQW) || d->qn.ensure(4 * R)) return ORBX_EDEVICE;
    KD_CHK(hipMemsetAsync(d->qn.p, 0, 4 * R, d->stream));
    for (auto &s : d->q) s.staged = false;
    return ORBX_OK;
}

// Reallocate-and-copy growth of a state buffer that has no host mirror
int grow_copy(DevBuf &b, size_t old_bytes, size_t new_bytes, hipStream_t st) {
    DevBuf nb;
    if (nb.ensure(new_bytes)) return ORBX_EDEVICE;
    if (b.p && old_bytes) KD_CHK(hipMemcpyAsync(nb.p, b.p, old_bytes, hipMemcpyDeviceToDevice, st));
    KD_CHK(hipStreamSynchronize(st));
    b.release();
    b = nb;
    return ORBX_OK;
}

int ensure_slots(orbd_db *d, int need) {
    if (need <= d->slot_cap) return ORBX_OK;
    const int cap = std::max(std::max(need, 64), 2 * d->slot_cap);
    if (d->d_meta.ensure(sizeof(KfMeta) * (size_t)cap)) return ORBX_EDEVICE;   // re-uploaded from the host mirror
    if (d->hi) KD_CHK(hipMemcpyAsync(d->d_meta.p, d->meta.data(), sizeof(KfMeta) * (size_t)d->hi, hipMemcpyHostToDevice, d->stream));
    const int rc = grow_copy(d->d_reloc, 4 * (size_t)d->hi, 4 * (size_t)cap, d->stream);
    if (rc) return rc;
    d->slot_cap = cap;
    d->cov_dirty = true;
    return ORBX_OK;
}

// Room for n more words: a new pool of twice the live size, the live BowVectors copied to its front
int ensure_pool(orbd_db *d, size_t n) {
    if (d->pool_used + n <= d->pool_cap) return ORBX_OK;
    const size_t cap = std::max<size_t>(2 * (d->live_words + n), 1 << 16);
    DevBuf nw, nv;
    if (nw.ensure(4 * cap) || nv.ensure(8 * cap)) { nw.release(); nv.release(); return ORBX_EDEVICE; }
    size_t used = 0;
    for (int s = 0; s < d->hi; s++) {
        KfMeta &m = d->meta[s];
        if (m.len < 0) continue;
        if (m.len > 0) {
            KD_CHK(hipMemcpyAsync((uint32_t *)nw.p + used, (uint32_t *)d->pool_w.p + m.off, 4 * (size_t)m.len, hipMemcpyDeviceToDevice, d->stream));
            KD_CHK(hipMemcpyAsync((double *)nv.p + used, (double *)d->pool_v.p + m.off, 8 * (size_t)m.len, hipMemcpyDeviceToDevice, d->stream));
        }
        m.off = (long long)used;
        used += (size_t)m.len;
    }
    if (d->hi) KD_CHK(hipMemcpyAsync(d->d_meta.p, d->meta.data(), sizeof(KfMeta) * (size_t)d->hi, hipMemcpyHostToDevice, d->stream));
    KD_CHK(hipStreamSynchronize(d->stream));
    d->pool_w.release();
    d->pool_v.release();
    d->pool_w = nw;
    d->pool_v = nv;
    d->pool_used = used;
    d->pool_cap = cap;
    return ORBX_OK;
}

bool words_ok(const orbd_db *d, const uint32_t *words, const double *values, int n) {
    if (n < 0 || n > kQW || (n > 0 && (!words || !values))) return false;
    for (int i = 0; i < n; i++)
        if (words[i] >= (uint32_t)d->n_words || (i > 0 && words[i] <= words[i - 1])) return false;
    return true;
}

// A free slot with its bookkeeping, the BowVector's place in the pool reserved; *slot's meta is uploaded by the caller
int new_slot(orbd_db *d, long long kf_id, int n, int *slot) {
    if (d->next_seq == 0xffffffffu) return ORBX_ESTATE;
    int rc = ensure_pool(d, (size_t)n);
    if (rc) return rc;
    int s;
    if (!d->free_slots.empty()) {
        s = d->free_slots.back();
        d->free_slots.pop_back();
    } else {
        rc = ensure_slots(d, d->hi + 1);
        if (rc) return rc;
        s = d->hi++;
        d->meta.push_back(KfMeta{});
        d->cov.emplace_back();
    }
    KfMeta &m = d->meta[s];
    m.off = (long long)d->pool_used;
    m.id = kf_id;
    m.seq = d->next_seq++;
    m.len = n;
    d->pool_used += (size_t)n;
    d->live_words += (size_t)n;
    d->cov[s].clear();
    d->slot_of[kf_id] = s;
    d->cov_dirty = true;
    *slot = s;
    return ORBX_OK;
}

int upload_slot(orbd_db *d, int s) {
    KD_CHK(hipMemcpyAsync((KfMeta *)d->d_meta.p + s, &d->meta[s], sizeof(KfMeta), hipMemcpyHostToDevice, d->stream));
    KD_CHK(hipMemsetAsync((float *)d->d_reloc.p + s, 0, 4, d->stream));   // mRelocScore of a new keyframe: 0.0f
    return ORBX_OK;
}

int ensure_work(orbd_db *d) {
    const int rows = d->nq + 1, stride = std::max(d->slot_cap, 1);
    if (rows <= d->work_rows && stride <= d->work_stride) return ORBX_OK;
    const int R = std::max(rows, d->work_rows), S = std::max(stride, d->work_stride);
    const size_t n = (size_t)R * S;
    DevBuf *b4[] = {&d->cnt, &d->fw, &d->si, &d->tslot, &d->sm_slot, &d->best, &d->flag};
    for (DevBuf *b : b4) if (b->ensure(4 * n)) return ORBX_EDEVICE;
    if (d->tkey.ensure(8 * n) || d->d_in.ensure(row_in_bytes(S) * R) || d->d_out.ensure(row_out_bytes(S) * R)) return ORBX_EDEVICE;
    d->work_rows = R;
    d->work_stride = S;
    return ORBX_OK;
}

// Rows [row0, row0 + n) through the kernels on `st`: one upload of the queries' records, four launches, one
// download of the results into `out`; the caller waits
int run_rows(orbd_db *d, int row0, int n, HostRes &out, hipStream_t st) {
    int rc = ensure_work(d);
    if (!rc) rc = out.shape(n, d->work_stride);
    if (rc) return rc;
    const int stride = d->work_stride;
    std::memset(out.buf.p, 0, row_out_bytes(stride) * n);
    if (d->hi == 0) return ORBX_OK;   // an empty database: every query returns empty
    if (d->cov_dirty) {   // covisible ids -> slots; an id that is not in the database is skipped
        std::vector<int> tab((size_t)d->hi * kCov, -1);
        for (int s = 0; s < d->hi; s++) {
            if (d->meta[s].len < 0) continue;
            for (size_t j = 0; j < d->cov[s].size(); j++) {
                auto it = d->slot_of.find(d->cov[s][j]);
                if (it != d->slot_of.end()) tab[(size_t)s * kCov + j] = it->second;
            }
        }
        if (d->d_cov.ensure(4 * (size_t)d->slot_cap * kCov)) return ORBX_EDEVICE;
        KD_CHK(hipMemcpyAsync(d->d_cov.p, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice, d->stream));
        KD_CHK(hipStreamSynchronize(d->stream));
        d->cov_dirty = false;
    }
    const size_t in_bytes = row_in_bytes(stride) * n;
    if (d->h_in.ensure(in_bytes)) return ORBX_EDEVICE;
    std::memset(d->h_in.p, 0, in_bytes);
    for (int r = 0; r < n; r++) {
        const StagedQuery &sq = d->q[row0 + r];
        const RowIn I = row_in(d->h_in.p, stride, r);
        QHdr *qh = const_cast<QHdr *>(I.qh);
        uint8_t *excl = const_cast<uint8_t *>(I.excl);
        qh->kind = sq.kind;
        qh->min_score = sq.min_score;
        if (sq.kind == ORBD_LOOP)
            for (long long id : sq.connected) {
                auto it = d->slot_of.find(id);
                if (it != d->slot_of.end()) excl[it->second] = 1;
            }
    }
    KD_CHK(hipMemcpyAsync((char *)d->d_in.p + row_in_bytes(stride) * row0, d->h_in.p, in_bytes, hipMemcpyHostToDevice, st));
    ScoreArgs S{};
    S.pool_w = d->pool_w.as<uint32_t>(); S.pool_v = d->pool_v.as<double>(); S.meta = d->d_meta.as<KfMeta>();
    S.n_slots = d->hi;
    S.qw = d->qw.as<uint32_t>(); S.qv = d->qv.as<double>(); S.qn = d->qn.as<int>();
    S.row0 = row0;
    S.cnt = d->cnt.as<int>(); S.fw = d->fw.as<uint32_t>(); S.si = d->si.as<float>();
    S.row_stride = stride;
    S.q_cap = 1;
    for (int r = 0; r < n; r++) S.q_cap = std::max(S.q_cap, d->q[row0 + r].n_upper);
    kfdb_score_kernel<<<dim3((d->hi + kWaves - 1) / kWaves, n), 64 * kWaves, 12 * (size_t)S.q_cap, st>>>(S);
    SelArgs A{};
    A.meta = S.meta; A.n_slots = d->hi; A.in = d->d_in.p; A.out = d->d_out.p;
    A.cnt = S.cnt; A.fw = S.fw; A.si = S.si;
    A.tkey = d->tkey.as<unsigned long long>(); A.tslot = d->tslot.as<int>();
    A.sm_slot = d->sm_slot.as<int>(); A.best = d->best.as<int>(); A.flag = d->flag.as<int>();
    A.covis = d->d_cov.as<int>(); A.reloc_score = d->d_reloc.as<float>();
    A.row_stride = stride; A.row0 = row0; A.n_rows = n;
    kfdb_select_kernel<<<n, kSelThreads, 0, st>>>(A);
    kfdb_groups_kernel<<<n, kSelThreads, 0, st>>>(A);
    kfdb_state_kernel<<<(d->hi + 255) / 256, 256, 0, st>>>(A);
    KD_CHK(hipGetLastError());
    KD_CHK(hipMemcpyAsync(out.buf.p, (char *)d->d_out.p + row_out_bytes(stride) * row0, row_out_bytes(stride) * n,
                          hipMemcpyDeviceToHost, st));
    return ORBX_OK;
}

bool result_ok(const orbd_result *r) { return r && r->cap >= 0 && (r->cap == 0 || r->candidates); }

int deliver(const HostRes &h, int row, orbd_result *r) {
    const RowOut O = row_out(h.buf.p, h.stride, row);
    const int4 hd = *O.hdr;
    r->n_scored = hd.x;
    r->n_candidates = hd.y;
    r->min_common_words = hd.z;
    r->max_common_words = hd.w;
    const bool lists = r->scored_ids || r->scored_si || r->scored_words || r->acc_score || r->acc_best;
    if (hd.y > r->cap || (lists && hd.x > r->cap)) return ORBX_ECAP;
    if (hd.y) std::memcpy(r->candidates, O.cand, 8 * (size_t)hd.y);
    if (hd.x) {
        if (r->scored_ids) std::memcpy(r->scored_ids, O.sm_id, 8 * (size_t)hd.x);
        if (r->scored_si) std::memcpy(r->scored_si, O.sm_si, 4 * (size_t)hd.x);
        if (r->scored_words) std::memcpy(r->scored_words, O.sm_words, 4 * (size_t)hd.x);
        if (r->acc_score) std::memcpy(r->acc_score, O.acc, 4 * (size_t)hd.x);
        if (r->acc_best) std::memcpy(r->acc_best, O.best_id, 8 * (size_t)hd.x);
    }
    return ORBX_OK;
}

bool query_ok(const orbd_db *d, const orbd_query *q, bool with_vector) {
    if (!q || (q->kind != ORBD_LOOP && q->kind != ORBD_RELOC)) return false;
    if (q->n_connected < 0 || (q->n_connected > 0 && !q->connected)) return false;
    return !with_vector || words_ok(d, q->words, q->values, q->n);
}

void note_query(orbd_db *d, int row, const orbd_query *q, int n_upper) {
    StagedQuery &s = d->q[row];
    s.staged = true;
    s.n_upper = n_upper;
    s.kind = q->kind;
    s.min_score = q->kind == ORBD_LOOP ? q->min_score : 0.0f;
    s.connected.assign(q->connected, q->connected + (q->kind == ORBD_LOOP ? q->n_connected : 0));
}

int upload_query(orbd_db *d, int row, const uint32_t *words, const double *values, int n) {
    int rc = ensure_device(d);
    if (!rc) rc = ensure_query_rows(d);
    if (rc) return rc;
    const int32_t nn = n;
    hipStream_t st = d->stream;
    if (n) {
        KD_CHK(hipMemcpyAsync((uint32_t *)d->qw.p + (size_t)row * kQW, words, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        KD_CHK(hipMemcpyAsync((double *)d->qv.p + (size_t)row * kQW, values, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    }
    KD_CHK(hipMemcpyAsync((int *)d->qn.p + row, &nn, 4, hipMemcpyHostToDevice, st));
    KD_CHK(hipStreamSynchronize(st));   // the caller's arrays are free on return
    return ORBX_OK;
}

// the vocabulary's frame checked against this database, without touching a device
bool vocab_ok(const orbd_db *d, orbv_vocab *v, int frame, BowBatchView *bv) {
    return v && bow_batch_view(v, frame, bv) == 0 && bv->voc_words <= d->n_words && bv->cap <= kQW;
}

}  // namespace

extern "C" {

int orbd_create(int n_words, int scoring, orbd_db **out) {
    if (!out || n_words < 1 || scoring != ORBD_L1_NORM) return ORBX_EINVAL;
    orbd_db *d = new orbd_db();
    d->n_words = n_words;
    d->q.resize(1);
    *out = d;
    return ORBX_OK;
}

void orbd_destroy(orbd_db *d) {
    if (!d) return;
    if (d->dev_ready) {
        (void)hipSetDevice(d->device);
        if (d->done) { (void)hipEventSynchronize(d->done); (void)hipEventDestroy(d->done); }
        if (d->stream) { (void)hipStreamSynchronize(d->stream); (void)hipStreamDestroy(d->stream); }
        d->batch.buf.release();
        d->single.buf.release();
        d->h_in.release();
        DevBuf *bufs[] = {&d->pool_w, &d->pool_v, &d->d_meta, &d->d_cov, &d->d_reloc, &d->qw, &d->qv, &d->qn, &d->d_in,
                          &d->d_out, &d->cnt, &d->fw, &d->si, &d->tkey, &d->tslot, &d->sm_slot, &d->best, &d->flag,
                          &d->sc_list, &d->sc_cnt, &d->sc_fw, &d->sc_si};
        for (DevBuf *b : bufs) b->release();
    }
    delete d;
}

int orbd_add(orbd_db *d, int64_t kf_id, const uint32_t *words, const double *values, int n) {
    if (!d || kf_id < 0) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (!words_ok(d, words, values, n) || d->slot_of.count(kf_id)) return ORBX_EINVAL;
    int rc = ensure_device(d), s = 0;
    if (!rc) rc = settle(d);
    if (!rc) rc = new_slot(d, kf_id, n, &s);
    if (rc) return rc;
    const KfMeta &m = d->meta[s];
    if (n) {
        KD_CHK(hipMemcpyAsync((uint32_t *)d->pool_w.p + m.off, words, 4 * (size_t)n, hipMemcpyHostToDevice, d->stream));
        KD_CHK(hipMemcpyAsync((double *)d->pool_v.p + m.off, values, 8 * (size_t)n, hipMemcpyHostToDevice, d->stream));
    }
    rc = upload_slot(d, s);
    if (rc) return rc;
    KD_CHK(hipStreamSynchronize(d->stream));
    return ORBX_OK;
}

int orbd_add_from_vocab(orbd_db *d, int64_t kf_id, orbv_vocab *v, int frame) {
    if (!d || kf_id < 0) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    BowBatchView bv;
    if (!vocab_ok(d, v, frame, &bv) || d->slot_of.count(kf_id)) return ORBX_EINVAL;
    int rc = ensure_device(d), s = 0;
    if (!rc) rc = settle(d);
    if (rc) return rc;
    // the BowVector's length decides its place in the pool: 4 bytes come back, the vector itself stays in HBM
    KD_CHK(hipStreamWaitEvent(d->stream, bv.done, 0));
    int32_t n = 0;
    KD_CHK(d2h_sync(&n, bv.n_words, 4, d->stream));
    if (n < 0 || n > bv.cap) return ORBX_ESTATE;
    rc = new_slot(d, kf_id, n, &s);
    if (rc) return rc;
    const KfMeta &m = d->meta[s];
    if (n) {
        KD_CHK(hipMemcpyAsync((uint32_t *)d->pool_w.p + m.off, bv.words, 4 * (size_t)n, hipMemcpyDeviceToDevice, d->stream));
        KD_CHK(hipMemcpyAsync((double *)d->pool_v.p + m.off, bv.values, 8 * (size_t)n, hipMemcpyDeviceToDevice, d->stream));
    }
    rc = upload_slot(d, s);
    if (rc) return rc;
    KD_CHK(hipStreamSynchronize(d->stream));
    return ORBX_OK;
}

int orbd_erase(orbd_db *d, int64_t kf_id) {
    if (!d) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    auto it = d->slot_of.find(kf_id);
    if (it == d->slot_of.end()) return ORBX_EINVAL;
    const int s = it->second;
    int rc = ensure_device(d);   // a known id was added: the device is there
    if (!rc) rc = settle(d);
    if (rc) return rc;
    d->live_words -= (size_t)d->meta[s].len;
    d->meta[s].len = -1;
    d->cov[s].clear();
    d->slot_of.erase(it);
    d->free_slots.push_back(s);
    d->cov_dirty = true;
    KD_CHK(hipMemcpyAsync((KfMeta *)d->d_meta.p + s, &d->meta[s], sizeof(KfMeta), hipMemcpyHostToDevice, d->stream));
    KD_CHK(hipStreamSynchronize(d->stream));
    return ORBX_OK;
}

int orbd_clear(orbd_db *d) {
    if (!d) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    const int rc = settle(d);
    if (rc) return rc;
    d->slot_of.clear();
    d->meta.clear();
    d->cov.clear();
    d->free_slots.clear();
    d->hi = 0;
    d->pool_used = d->live_words = 0;
    d->cov_dirty = true;
    return ORBX_OK;
}

int orbd_size(orbd_db *d, int32_t *n) {
    if (!d || !n) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    *n = (int32_t)d->slot_of.size();
    return ORBX_OK;
}

int orbd_set_covisibles(orbd_db *d, int64_t kf_id, const int64_t *ids, int n) {
    if (!d || n < 0 || n > kCov || (n > 0 && !ids)) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    auto it = d->slot_of.find(kf_id);
    if (it == d->slot_of.end()) return ORBX_EINVAL;
    d->cov[it->second].assign(ids, ids + n);
    d->cov_dirty = true;
    return ORBX_OK;
}

int orbd_detect(orbd_db *d, const orbd_query *q, orbd_result *r) {
    if (!d || !result_ok(r)) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (!query_ok(d, q, true)) return ORBX_EINVAL;
    int rc = settle(d);
    if (!rc) rc = upload_query(d, d->nq, q->words, q->values, q->n);
    if (rc) return rc;
    note_query(d, d->nq, q, q->n);
    rc = run_rows(d, d->nq, 1, d->single, d->stream);
    if (rc) return rc;
    KD_CHK(hipStreamSynchronize(d->stream));
    return deliver(d->single, 0, r);
}

int orbd_reserve(orbd_db *d, int n_slots) {
    if (!d || n_slots < 1 || n_slots > 65535) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (settle(d)) return ORBX_EDEVICE;
    d->nq = n_slots;
    d->q.assign((size_t)n_slots + 1, StagedQuery{});
    d->batch.rows = 0;
    if (d->qw.p) (void)hipSetDevice(d->device);
    if (d->qw.p && d->qw.bytes < 4 * ((size_t)n_slots + 1) * kQW) {   // re-sized by the next call that reaches the device
        d->qw.release();
    } else if (d->qw.p) {
        if (hipMemsetAsync(d->qn.p, 0, 4 * ((size_t)n_slots + 1), d->stream) != hipSuccess) return ORBX_EDEVICE;
    }
    return ORBX_OK;
}

int orbd_stage(orbd_db *d, int slot, const orbd_query *q) {
    if (!d) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (slot < 0 || slot >= d->nq || !query_ok(d, q, true)) return ORBX_EINVAL;
    int rc = settle(d);
    if (!rc) rc = upload_query(d, slot, q->words, q->values, q->n);
    if (rc) return rc;
    note_query(d, slot, q, q->n);
    return ORBX_OK;
}

int orbd_stage_from_vocab(orbd_db *d, int slot, const orbd_query *q, orbv_vocab *v, int frame) {
    if (!d) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    BowBatchView bv;
    if (slot < 0 || slot >= d->nq || !query_ok(d, q, false) || !vocab_ok(d, v, frame, &bv)) return ORBX_EINVAL;
    int rc = ensure_device(d);
    if (!rc) rc = settle(d);
    if (!rc) rc = ensure_query_rows(d);
    if (rc) return rc;
    hipStream_t st = d->stream;
    KD_CHK(hipStreamWaitEvent(st, bv.done, 0));
    // the whole row of the vocabulary's batch buffer: its length stays on the device with it
    KD_CHK(hipMemcpyAsync((uint32_t *)d->qw.p + (size_t)slot * kQW, bv.words, 4 * (size_t)bv.cap, hipMemcpyDeviceToDevice, st));
    KD_CHK(hipMemcpyAsync((double *)d->qv.p + (size_t)slot * kQW, bv.values, 8 * (size_t)bv.cap, hipMemcpyDeviceToDevice, st));
    KD_CHK(hipMemcpyAsync((int *)d->qn.p + slot, bv.n_words, 4, hipMemcpyDeviceToDevice, st));
    KD_CHK(hipStreamSynchronize(st));   // the vocabulary may overwrite its batch buffers after this call
    note_query(d, slot, q, bv.cap);
    return ORBX_OK;
}

int orbd_run_batch(orbd_db *d, int n_slots, void *stream) {
    if (!d) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (n_slots < 1 || n_slots > d->nq) return ORBX_EINVAL;
    for (int s = 0; s < n_slots; s++)
        if (!d->q[s].staged) return ORBX_ESTATE;
    if (!d->dev_ready) return ORBX_ESTATE;
    KD_CHK(hipSetDevice(d->device));
    int rc = settle(d);
    if (rc) return rc;
    d->batch.rows = 0;
    hipStream_t st = stream ? (hipStream_t)stream : d->stream;
    rc = run_rows(d, 0, n_slots, d->batch, st);
    if (rc) { d->batch.rows = 0; return rc; }
    KD_CHK(hipEventRecord(d->done, st));
    d->pending = true;
    return ORBX_OK;
}

int orbd_fetch(orbd_db *d, int slot, orbd_result *r) {
    if (!d || !result_ok(r)) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (slot < 0 || slot >= d->nq) return ORBX_EINVAL;
    if (slot >= d->batch.rows) return ORBX_ESTATE;
    const int rc = settle(d);
    return rc ? rc : deliver(d->batch, slot, r);
}

int orbd_scores(orbd_db *d, const uint32_t *words, const double *values, int n, const int64_t *kf_ids, int n_ids,
                float *scores, float *min_score) {
    if (!d || !min_score || n_ids < 0 || (n_ids > 0 && (!kf_ids || !scores))) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(d->mu);
    if (!words_ok(d, words, values, n)) return ORBX_EINVAL;
    std::vector<int> list, where;
    for (int i = 0; i < n_ids; i++) {
        scores[i] = -1.0f;   // not in the database: skipped, as a keyframe with isBad() is
        auto it = d->slot_of.find(kf_ids[i]);
        if (it != d->slot_of.end()) { list.push_back(it->second); where.push_back(i); }
    }
    *min_score = 1.0f;
    if (list.empty()) return ORBX_OK;
    int rc = settle(d);
    if (!rc) rc = upload_query(d, d->nq, words, values, n);
    if (rc) return rc;
    const size_t m = list.size();
    if (d->sc_list.ensure(4 * m) || d->sc_cnt.ensure(4 * m) || d->sc_fw.ensure(4 * m) || d->sc_si.ensure(4 * m)) return ORBX_EDEVICE;
    hipStream_t st = d->stream;
    KD_CHK(hipMemcpyAsync(d->sc_list.p, list.data(), 4 * m, hipMemcpyHostToDevice, st));
    ScoreArgs S{};
    S.pool_w = d->pool_w.as<uint32_t>(); S.pool_v = d->pool_v.as<double>(); S.meta = d->d_meta.as<KfMeta>();
    S.n_slots = d->hi;
    S.qw = d->qw.as<uint32_t>(); S.qv = d->qv.as<double>(); S.qn = d->qn.as<int>();
    S.row0 = d->nq;
    S.slot_list = d->sc_list.as<int>(); S.n_list = (int)m;
    S.cnt = d->sc_cnt.as<int>(); S.fw = d->sc_fw.as<uint32_t>(); S.si = d->sc_si.as<float>();
    S.q_cap = std::max(n, 1);
    kfdb_score_kernel<<<dim3(((int)m + kWaves - 1) / kWaves, 1), 64 * kWaves, 12 * (size_t)S.q_cap, st>>>(S);
    KD_CHK(hipGetLastError());
    std::vector<float> si(m);
    KD_CHK(d2h_sync(si.data(), d->sc_si.p, 4 * m, st));
    for (size_t i = 0; i < m; i++) {
        scores[where[i]] = si[i];
        if (si[i] < *min_score) *min_score = si[i];
    }
    return ORBX_OK;
}

}  // extern "C"
