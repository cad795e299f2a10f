// Driver of the C++ host layer's Optimizer::OptimizeSim3 / OptimizeSim3All and of the Sim3 value type
// (tests/test_sim3opt_cpp_gpu.py).
//
//   optimize_sim3_test <in.bin> <out.bin>
//
// in.bin : int32 mN1, int32 fix_scale, float th2, float K1[4], K2[4], float R1w[9], t1w[3], R2w[9], t2w[3],
//          double S12[8] (q xyzw, t, s), int32 flags[mN1] (1 pMP2, 2 pMP1, 4 bad1, 8 bad2), int32 indexKF2[mN1],
//          octave1[mN1], octave2[mN1], float Xw1[mN1][3], Xw2[mN1][3], pt1[mN1][2], pt2[mN1][2];
//          then for the value type: double A[8], B[8], R[9], X[3].
// out.bin: arrays as (int64 count, data): int32 nIn[4] (OptimizeSim3; OptimizeSim3All over the same candidate
//          twice, which must reproduce it in both slots; OptimizeSim3 with th2 = 0); uint8 pMP2 after
//          OptimizeSim3; double g2oS12[8] after it; uint8 pMP2 and double g2oS12[8] after the th2 = 0 call
//          (every pair removed after the first optimize: `return 0`, g2oS12 not written);
//          double A*B [8], A.inverse() [8], A.map(X) [3], Sim3(R, t_A, s_A) [8], Sim3() [8].
#include <cstdio>
#include <cstring>
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

static std::vector<double> flat(const Sim3 &S) {
    return {S.rotation()[0], S.rotation()[1], S.rotation()[2], S.rotation()[3], S.translation()[0], S.translation()[1],
            S.translation()[2], S.scale()};
}

static Sim3 unflat(const double *v) { return Sim3::FromQuaternion(v, v + 4, v[7]); }

static std::vector<uint8_t> mask(const std::vector<Sim3Match> &m) {
    std::vector<uint8_t> r(m.size());
    for (size_t i = 0; i < m.size(); i++) r[i] = m[i].pMP2 ? 1 : 0;
    return r;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    try {
        const std::vector<char> blob = slurp(argv[1]);
        Reader rd{blob.data(), blob.data() + blob.size()};
        const int mN1 = *rd.take<int32_t>(1);
        const int fix = *rd.take<int32_t>(1);
        const float th2 = *rd.take<float>(1);
        const float *K1 = rd.take<float>(4), *K2 = rd.take<float>(4);
        const float *R1 = rd.take<float>(9), *t1 = rd.take<float>(3), *R2 = rd.take<float>(9), *t2 = rd.take<float>(3);
        const double *S12 = rd.take<double>(8);
        const int32_t *flags = rd.take<int32_t>(mN1), *i2 = rd.take<int32_t>(mN1);
        const int32_t *o1 = rd.take<int32_t>(mN1), *o2 = rd.take<int32_t>(mN1);
        const float *X1 = rd.take<float>((size_t)mN1 * 3), *X2 = rd.take<float>((size_t)mN1 * 3);
        const float *p1 = rd.take<float>((size_t)mN1 * 2), *p2 = rd.take<float>((size_t)mN1 * 2);
        const double *A8 = rd.take<double>(8), *B8 = rd.take<double>(8), *R = rd.take<double>(9), *X = rd.take<double>(3);

        Sim3KeyFrame kf1, kf2;
        kf1.fx = K1[0]; kf1.fy = K1[1]; kf1.cx = K1[2]; kf1.cy = K1[3];
        kf2.fx = K2[0]; kf2.fy = K2[1]; kf2.cx = K2[2]; kf2.cy = K2[3];
        memcpy(kf1.Rcw, R1, 36); memcpy(kf1.tcw, t1, 12);
        memcpy(kf2.Rcw, R2, 36); memcpy(kf2.tcw, t2, 12);
        std::vector<float> inv(8);
        float sf = 1.0f;
        for (int i = 0; i < 8; i++) {   // mvInvLevelSigma2 of ORBextractor(…, 1.2f, 8, …)
            inv[i] = 1.0f / (sf * sf);
            sf = sf * 1.2f;
        }
        kf1.mvInvLevelSigma2 = kf2.mvInvLevelSigma2 = inv;
        std::vector<Sim3Match> m(mN1);
        for (int i = 0; i < mN1; i++) {
            m[i].pMP2 = flags[i] & 1;
            m[i].pMP1 = flags[i] & 2;
            m[i].bad1 = flags[i] & 4;
            m[i].bad2 = flags[i] & 8;
            m[i].indexKF1 = i;
            m[i].indexKF2 = i2[i];
            m[i].octave1 = o1[i];
            m[i].octave2 = o2[i];
            memcpy(m[i].Xw1, X1 + 3 * i, 12);
            memcpy(m[i].Xw2, X2 + 3 * i, 12);
            memcpy(m[i].pt1, p1 + 2 * i, 8);
            memcpy(m[i].pt2, p2 + 2 * i, 8);
        }

        std::vector<Sim3Match> ma = m;
        Sim3 Sa = unflat(S12);
        const int nIn = Optimizer::OptimizeSim3(kf1, kf2, ma, Sa, th2, fix != 0);

        // batched: the same candidate in two slots
        std::vector<Sim3Match> mb = m, mc = m;
        std::vector<Sim3> vS{unflat(S12), unflat(S12)};
        std::vector<int> vn;
        Optimizer::OptimizeSim3All(kf1, {&kf2, &kf2}, {&mb, &mc}, vS, th2, fix != 0, vn);
        if (mask(mb) != mask(ma) || flat(vS[0]) != flat(Sa)) throw std::runtime_error("OptimizeSim3All[0] != OptimizeSim3");
        if (mask(mc) != mask(ma) || flat(vS[1]) != flat(Sa)) throw std::runtime_error("OptimizeSim3All[1] != OptimizeSim3");
        std::vector<Sim3Match> md = m;
        Sim3 Sd = unflat(S12);
        const int nZero = Optimizer::OptimizeSim3(kf1, kf2, md, Sd, 0.0f, fix != 0);

        const Sim3 A = unflat(A8), B = unflat(B8);
        double mapped[3];
        A.map(X, mapped);
        FILE *f = fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        put(f, std::vector<int32_t>{nIn, vn[0], vn[1], nZero});
        put(f, mask(ma));
        put(f, flat(Sa));
        put(f, mask(md));
        put(f, flat(Sd));
        put(f, flat(A * B));
        put(f, flat(A.inverse()));
        put(f, std::vector<double>(mapped, mapped + 3));
        put(f, flat(Sim3(R, A.translation(), A.scale())));
        put(f, flat(Sim3()));
        fclose(f);
    } catch (const std::exception &e) {
        fprintf(stderr, "optimize_sim3_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
