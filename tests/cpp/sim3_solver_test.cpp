// Driver of the C++ host class orbslam2_amd::Sim3Solver (tests/test_sim3solver_cpp_gpu.py):
// builds the solvers of one LoopClosing::ComputeSim3 call from a blob of candidates, evaluates
// them with one EvaluateAll launch and runs the reference's round-robin of iterate(5) calls
// (LoopClosing.cc:378-404) with an injected, deterministic RandomInt.
//
//   sim3_solver_test <in.bin> <out.bin> <seed> [repeats]
//
// repeats > 1 (tools/sim3_bench.py) runs the whole call that many times from the same seed and
// reports the last one, so the wall time excludes the first call's device set-up.
//
// in.bin : int32 n_candidates, then per candidate: int32 mN1, int32 fix_scale, float K1[4], K2[4],
//          int32 flags[mN1] (1 pMP2, 2 pMP1, 4 bad1, 8 bad2), int32 indexKF1[mN1], indexKF2[mN1],
//          octave1[mN1], octave2[mN1], float Xw1[mN1][3], Xw2[mN1][3] (both keyframes at the identity
//          pose, so X3Dc = Xw exactly).
// out.bin: arrays as (int64 count, data): int32 summary[5] = winner, its iteration (0-based), nInliers,
//          iterate() calls, wall microseconds of EvaluateAll + the round-robin; int32 per candidate
//          (N, mRansacMaxIts, mnIterations)[]; int32 triplets of all candidates concatenated;
//          uint8 vbInliers of the winner; float T12[16]; float R[9] t[3] s[1] from GetEstimated*;
//          int32 mvnMaxError1 of candidate 0.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "orbslam2_amd.hpp"

using namespace orbslam2_amd;

static std::vector<char> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> b(n);
    if (n && fread(b.data(), 1, n, f) != (size_t)n) throw std::runtime_error("short read");
    fclose(f);
    return b;
}

template <class T> static void put(FILE *f, const std::vector<T> &v) {
    const int64_t n = (int64_t)v.size();
    fwrite(&n, 8, 1, f);
    if (n) fwrite(v.data(), sizeof(T), v.size(), f);
}

struct Reader {
    const char *p, *end;
    template <class T> const T *take(size_t n) {
        if (p + n * sizeof(T) > end) throw std::runtime_error("blob too short");
        const T *r = reinterpret_cast<const T *>(p);
        p += n * sizeof(T);
        return r;
    }
};

// one ComputeSim3 call; out == NULL: a warm-up repeat, nothing written
static void run(const std::vector<char> &blob, uint32_t seed, const char *out) {
    Reader rd{blob.data(), blob.data() + blob.size()};
    const int nc = *rd.take<int32_t>(1);
    // one generator shared by the solvers, as the reference's rand() is
    uint32_t state = seed;
    Sim3Solver::RandomIntFn rnd = [&state](int lo, int hi) {
        state = (state * 1103515245u + 12345u) & 0x7fffffffu;
        return lo + (int)((state >> 8) % (uint32_t)(hi - lo + 1));
    };
    std::vector<float> sigma2(8);
    float sf = 1.0f;
    for (int i = 0; i < 8; i++) {   // mvLevelSigma2 of ORBextractor(…, 1.2f, 8, …)
        sigma2[i] = sf * sf;
        sf = sf * 1.2f;
    }
    std::vector<std::unique_ptr<Sim3Solver>> owners;
    std::vector<Sim3Solver *> vpSim3Solvers;
    for (int c = 0; c < nc; c++) {
        const int mN1 = *rd.take<int32_t>(1);
        const int fix = *rd.take<int32_t>(1);
        const float *K1 = rd.take<float>(4), *K2 = rd.take<float>(4);
        const int32_t *flags = rd.take<int32_t>(mN1), *i1 = rd.take<int32_t>(mN1), *i2 = rd.take<int32_t>(mN1);
        const int32_t *o1 = rd.take<int32_t>(mN1), *o2 = rd.take<int32_t>(mN1);
        const float *X1 = rd.take<float>((size_t)mN1 * 3), *X2 = rd.take<float>((size_t)mN1 * 3);
        Sim3KeyFrame kf1, kf2;
        kf1.fx = K1[0]; kf1.fy = K1[1]; kf1.cx = K1[2]; kf1.cy = K1[3];
        kf2.fx = K2[0]; kf2.fy = K2[1]; kf2.cx = K2[2]; kf2.cy = K2[3];
        kf1.mvLevelSigma2 = kf2.mvLevelSigma2 = sigma2;
        std::vector<Sim3Match> m(mN1);
        for (int i = 0; i < mN1; i++) {
            m[i].pMP2 = flags[i] & 1;
            m[i].pMP1 = flags[i] & 2;
            m[i].bad1 = flags[i] & 4;
            m[i].bad2 = flags[i] & 8;
            m[i].indexKF1 = i1[i];
            m[i].indexKF2 = i2[i];
            m[i].octave1 = o1[i];
            m[i].octave2 = o2[i];
            memcpy(m[i].Xw1, X1 + 3 * i, 12);
            memcpy(m[i].Xw2, X2 + 3 * i, 12);
        }
        owners.emplace_back(new Sim3Solver(kf1, kf2, m, fix != 0, rnd));
        owners.back()->SetRansacParameters(0.99, 20, 300);   // LoopClosing.cc:366
        vpSim3Solvers.push_back(owners.back().get());
    }
    const auto t0 = std::chrono::steady_clock::now();
    Sim3Solver::EvaluateAll(vpSim3Solvers);
    // LoopClosing.cc:378-416 up to the first returned Sim3
    std::vector<bool> vbDiscarded(nc, false), vbInliers;
    int nCandidates = nc, winner = -1, nInliers = 0, calls = 0;
    float T12[16] = {0};
    while (nCandidates > 0 && winner < 0) {
        for (int i = 0; i < nc && winner < 0; i++) {
            if (vbDiscarded[i]) continue;
            bool bNoMore;
            std::vector<bool> inl;
            int nin;
            const bool found = vpSim3Solvers[i]->iterate(5, bNoMore, inl, nin, T12);
            calls++;
            if (bNoMore) {
                vbDiscarded[i] = true;
                nCandidates--;
            }
            if (found) {
                winner = i;
                nInliers = nin;
                vbInliers = inl;
            }
        }
    }
    const int us = (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (!out) return;
    std::vector<int32_t> summary{winner, winner >= 0 ? vpSim3Solvers[winner]->GetIterations() - 1 : -1, nInliers, calls, us};
    std::vector<int32_t> per, trips, thr0;
    for (Sim3Solver *s : vpSim3Solvers) {
        per.push_back(s->GetNumCorrespondences());
        per.push_back(s->GetMaxIterations());
        per.push_back(s->GetIterations());
        trips.insert(trips.end(), s->GetTriplets().begin(), s->GetTriplets().end());
    }
    for (size_t v : vpSim3Solvers[0]->GetMaxError1()) thr0.push_back((int32_t)v);
    std::vector<uint8_t> inl8(vbInliers.begin(), vbInliers.end());
    std::vector<float> T(T12, T12 + 16), Rts(13, 0.0f);
    if (winner >= 0) {
        vpSim3Solvers[winner]->GetEstimatedRotation(Rts.data());
        vpSim3Solvers[winner]->GetEstimatedTranslation(Rts.data() + 9);
        Rts[12] = vpSim3Solvers[winner]->GetEstimatedScale();
    }
    FILE *f = fopen(out, "wb");
    if (!f) throw std::runtime_error("cannot write output");
    put(f, summary);
    put(f, per);
    put(f, trips);
    put(f, inl8);
    put(f, T);
    put(f, Rts);
    put(f, thr0);
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) {
        fprintf(stderr, "usage: %s in.bin out.bin seed [repeats]\n", argv[0]);
        return 2;
    }
    try {
        const std::vector<char> blob = slurp(argv[1]);
        const int reps = argc == 5 ? std::max(1, atoi(argv[4])) : 1;
        for (int rep = 0; rep < reps; rep++) run(blob, (uint32_t)atoi(argv[3]), rep + 1 == reps ? argv[2] : nullptr);
    } catch (const std::exception &e) {
        fprintf(stderr, "sim3_solver_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
