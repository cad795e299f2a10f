// C++ host layer over the orbslam2_amd C-ABI, mirroring the reference classes the HIP path
// replaces (same names, argument meaning and call order; OpenCV types swapped for PODs so
// this header builds without OpenCV). INTEGRATION.md shows the cv::Mat adapters that drop
// these into the reference tree unchanged for Tracking.cc / LocalMapping.cc.
//
//   orbslam2_amd::ORBextractor   <- ORB_SLAM2::ORBextractor (include/ORBextractor.h:80-216)
//   orbslam2_amd::ORBmatcher     <- ORB_SLAM2::ORBmatcher   (include/ORBmatcher.h:57-65, 169)
//   orbslam2_amd::ComputeStereoMatches <- Frame::ComputeStereoMatches (Frame.cc:831-1128)
//   orbslam2_amd::Optimizer::LocalBundleAdjustment <- Optimizer.h:112 (graph supplied flat)
//   orbslam2_amd::Optimizer::PoseOptimization     <- Optimizer.h:105 (edges supplied flat)
//   orbslam2_amd::ORBmatcher::SearchByProjection   <- ORBmatcher.h:82 (+ Frame::isInFrustum),
//                                                     ORBmatcher.h:102 (motion model)
//   orbslam2_amd::ORBVocabulary                    <- DBoW2 TemplatedVocabulary<FORB>:
//                                                     loadFromTextFile + transform (ComputeBoW)
//   orbslam2_amd::Sim3Solver                        <- ORB_SLAM2::Sim3Solver (include/Sim3Solver.h:40-170)
//   orbslam2_amd::KeyFrameDatabase                  <- ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h)
//   orbslam2_amd::LoopClosing::DetectLoop           <- LoopClosing.cc:137-285 (host logic over the database)
//
// Error behaviour: the reference has no error path (it asserts / returns silently); a GPU
// failure here throws std::runtime_error -- there is no CPU fallback.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbslam2_amd.h"

namespace orbslam2_amd {

using KeyPoint = orbx_kp;   // cv::KeyPoint memory layout: pt.x, pt.y, size, angle, response, octave, class_id

struct ImageU8 {            // cv::Mat CV_8UC1 view
    const uint8_t *data = nullptr;
    int cols = 0, rows = 0;
    int step = 0;           // bytes per row
};

inline void check(int rc, const char *what) {
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbslam2_amd: ") + what + " failed (" + std::to_string(rc) + ")");
}

class ORBextractor {
public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
        : nfeatures_(nfeatures), nlevels_(nlevels), scaleFactor_(scaleFactor) {
        orbx_params p{sizeof(orbx_params), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, /*resize_mode*/ 0, /*blur_mode*/ 0};
        check(orbx_create(&p, &h_), "orbx_create");
    }
    ~ORBextractor() { orbx_destroy(h_); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;

    // operator()(image, mask, keypoints, descriptors): descriptors is N x 32 bytes, row i
    // belongs to keypoints[i]. Empty image -> returns with outputs untouched (:1547).
    void operator()(const ImageU8 &image, std::vector<KeyPoint> &keypoints, std::vector<uint8_t> &descriptors) {
        if (!image.data || image.cols == 0 || image.rows == 0) return;
        const int cap = 2 * nfeatures_ + 512;
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(orbx_extract(h_, image.data, image.cols, image.rows, image.step, keypoints.data(), descriptors.data(), cap, &n),
              "orbx_extract");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }

    int GetLevels() const { return nlevels_; }
    float GetScaleFactor() const { return scaleFactor_; }
    std::vector<float> GetScaleFactors() const { return levels()[0]; }
    std::vector<float> GetInverseScaleFactors() const { return levels()[1]; }
    std::vector<float> GetScaleSigmaSquares() const { return levels()[2]; }
    std::vector<float> GetInverseScaleSigmaSquares() const { return levels()[3]; }

    // mvImagePyramid[level] (host copy of the device level)
    std::vector<uint8_t> ImagePyramidLevel(int level, int *cols, int *rows) {
        check(orbx_pyramid_level(h_, 0, level, nullptr, cols, rows), "orbx_pyramid_level");
        std::vector<uint8_t> out((size_t)(*cols) * (*rows));
        check(orbx_pyramid_level(h_, 0, level, out.data(), nullptr, nullptr), "orbx_pyramid_level");
        return out;
    }

    orbx_engine *engine() const { return h_; }

private:
    std::vector<std::vector<float>> levels() const {
        std::vector<std::vector<float>> v(4, std::vector<float>(nlevels_));
        int L = 0;
        check(orbx_levels(h_, &L, v[0].data(), v[1].data(), v[2].data(), v[3].data(), nullptr), "orbx_levels");
        return v;
    }
    orbx_engine *h_ = nullptr;
    int nfeatures_, nlevels_;
    float scaleFactor_;
};

// Frame::ComputeStereoMatches over the frame whose left/right images were last extracted by
// `left` / `right` (mvKeys = left keypoints, N = their count).
inline void ComputeStereoMatches(ORBextractor &left, ORBextractor &right, int N, float mbf, float mb,
                                 std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
    mvuRight.assign(N, -1.0f);
    mvDepth.assign(N, -1.0f);
    check(orbm_stereo_match(left.engine(), right.engine(), mbf, mb, mvuRight.data(), mvDepth.data(), N),
          "orbm_stereo_match");
}

// The Frame members SearchForInitialization reads (Frame.h): mvKeysUn, mDescriptors (N x 32)
// and the static image bounds mnMinX / mnMaxX / mnMinY / mnMaxY.
struct InitFrame {
    std::vector<KeyPoint> mvKeysUn;
    std::vector<uint8_t> mDescriptors;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
};

struct Point2f {   // cv::Point2f
    float x, y;
};

class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    ~ORBmatcher() { orbm_destroy(m_); }
    ORBmatcher(const ORBmatcher &) = delete;
    ORBmatcher &operator=(const ORBmatcher &) = delete;
    // DescriptorDistance (ORBmatcher.cc:2123-2143)
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b) {
        int d = 0;
        for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
        return d;
    }
    // brute-force best / second-best scan on the GPU
    static void HammingBest2(const std::vector<uint8_t> &q, const std::vector<uint8_t> &db, std::vector<int> &best,
                             std::vector<int> &bestDist, std::vector<int> &secondDist) {
        const int nq = (int)(q.size() / 32), ndb = (int)(db.size() / 32);
        best.resize(nq); bestDist.resize(nq); secondDist.resize(nq);
        check(orbm_hamming_best2(q.data(), nq, db.data(), ndb, best.data(), bestDist.data(), secondDist.data()),
              "orbm_hamming_best2");
    }
    // best / second over caller-built candidate lists (CSR: query i's candidates are
    // candIdx[candOff[i] .. candOff[i+1]) into db), first minimum in list order
    void HammingBest2(const std::vector<uint8_t> &q, const std::vector<uint8_t> &db, const std::vector<int32_t> &candOff,
                      const std::vector<int32_t> &candIdx, std::vector<int32_t> &best, std::vector<int32_t> &bestDist,
                      std::vector<int32_t> &secondDist) {
        const int nq = (int)(q.size() / 32), ndb = (int)(db.size() / 32);
        if ((int)candOff.size() != nq + 1) throw std::invalid_argument("candOff needs nq + 1 entries");
        best.resize(nq); bestDist.resize(nq); secondDist.resize(nq);
        check(orbm_hamming_best2_cand(handle(), q.data(), nq, db.data(), ndb, candOff.data(), candIdx.data(), best.data(),
                                      bestDist.data(), secondDist.data()),
              "orbm_hamming_best2_cand");
    }
    // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:580-748):
    // vbPrevMatched is read as the window centres and updated with the matched F2 positions.
    int SearchForInitialization(const InitFrame &F1, const InitFrame &F2, std::vector<Point2f> &vbPrevMatched,
                                std::vector<int> &vnMatches12, int windowSize = 10) {
        static_assert(sizeof(Point2f) == 8 && sizeof(int) == 4, "Point2f / int layout");
        const int n1 = (int)F1.mvKeysUn.size();
        vnMatches12.assign(n1, -1);
        if (vbPrevMatched.size() < (size_t)n1) throw std::invalid_argument("vbPrevMatched shorter than F1");
        if (F1.mDescriptors.size() < (size_t)n1 * 32 || F2.mDescriptors.size() < F2.mvKeysUn.size() * 32)
            throw std::invalid_argument("descriptors shorter than keypoints");
        const orbm_frame f1{n1, F1.mvKeysUn.data(), F1.mDescriptors.data(), F1.mnMinX, F1.mnMaxX, F1.mnMinY, F1.mnMaxY};
        const orbm_frame f2{(int32_t)F2.mvKeysUn.size(), F2.mvKeysUn.data(), F2.mDescriptors.data(), F2.mnMinX, F2.mnMaxX,
                            F2.mnMinY, F2.mnMaxY};
        int32_t nmatches = 0;
        check(orbm_search_for_initialization(handle(), &f1, &f2, reinterpret_cast<float *>(vbPrevMatched.data()),
                                             vnMatches12.data(), windowSize, &nmatches),
              "orbm_search_for_initialization");
        return nmatches;
    }
    // SearchByProjection(Frame&, const vector<MapPoint*>&, th) with the in-view selection of
    // Tracking::SearchLocalPoints (isInFrustum(pMP, 0.5)); owner[i] = index into M assigned to
    // keypoint i, -1 untouched. inView (optional) = mbTrackInView per map point.
    int SearchByProjection(const orbt_frame &F, const orbt_mappoints &M, float th, const uint8_t *blocked,
                           std::vector<int32_t> &owner, std::vector<uint8_t> *inView = nullptr) {
        owner.assign(F.n, -1);
        std::vector<uint8_t> iv(M.n);
        orbt_view v{iv.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
        int32_t nm = 0;
        check(orbt_search_local_points(track(), &F, &M, 0.5f, th, mfNNratio, blocked, &v, owner.data(), &nm),
              "orbt_search_local_points");
        if (inView) *inView = iv;
        return nm;
    }
    // SearchByProjection(CurrentFrame, LastFrame, th, bMono); owner[i] == -2: set to NULL by
    // the rotation-consistency check.
    int SearchByProjection(const orbt_frame &cur, const orbt_frame &last, const int32_t *lastMp,
                           const uint8_t *lastOutlier, const orbt_mappoints &M, float th, bool bMono,
                           std::vector<int32_t> &owner) {
        owner.assign(cur.n, -1);
        int32_t nm = 0;
        check(orbt_search_by_projection_frame(track(), &cur, &last, lastMp, lastOutlier, &M, th, bMono ? 1 : 0,
                                              mbCheckOrientation ? 1 : 0, nullptr, owner.data(), &nm),
              "orbt_search_by_projection_frame");
        return nm;
    }
    // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (Tracking::Relocalization):
    // kfMp = pKF->GetMapPointMatches() as indices into M, M.flags ORBT_MP_FOUND = sAlreadyFound
    int SearchByProjection(const orbt_frame &cur, const orbt_frame &kf, const int32_t *kfMp, const orbt_mappoints &M,
                           float th, int ORBdist, const uint8_t *blocked, std::vector<int32_t> &owner) {
        owner.assign(cur.n, -1);
        int32_t nm = 0;
        check(orbt_search_by_projection_keyframe(track(), &cur, &kf, kfMp, &M, th, ORBdist, mbCheckOrientation ? 1 : 0,
                                                 blocked, owner.data(), &nm),
              "orbt_search_by_projection_keyframe");
        return nm;
    }
    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (LoopClosing): vpMatched in/out as indices
    int SearchByProjection(const orbt_frame &kf, const float Scw[16], const orbt_mappoints &vpPoints,
                           std::vector<int32_t> &vpMatched, int th) {
        vpMatched.resize(kf.n, -1);
        int32_t nm = 0;
        check(orbt_search_by_projection_sim3(track(), &kf, Scw, &vpPoints, th, vpMatched.data(), &nm),
              "orbt_search_by_projection_sim3");
        return nm;
    }
    // SearchByBoW(pKF1, pKF2, vpMatches12) (LoopClosing::ComputeSim3)
    int SearchByBoW(const orbb_keyframe &kf1, const orbb_keyframe &kf2, std::vector<int32_t> &vpMatches12) {
        vpMatches12.assign(kf1.n, -1);
        int32_t nm = 0;
        check(orbb_search_by_bow_kf(bow(), &kf1, &kf2, mfNNratio, mbCheckOrientation ? 1 : 0, vpMatches12.data(), &nm),
              "orbb_search_by_bow_kf");
        return nm;
    }
    // SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th): vpMatches12 in/out as indices
    int SearchBySim3(const orbt_frame &kf1, const int32_t *kf1Mp, const orbt_frame &kf2, const int32_t *kf2Mp,
                     const orbt_mappoints &M, std::vector<int32_t> &vpMatches12, float s12, const float R12[9],
                     const float t12[3], float th) {
        vpMatches12.resize(kf1.n, -1);
        int32_t nf = 0;
        check(orbt_search_by_sim3(track(), &kf1, kf1Mp, &kf2, kf2Mp, &M, s12, R12, t12, th, vpMatches12.data(), &nf),
              "orbt_search_by_sim3");
        return nf;
    }
    // Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), search half: the caller applies the updates in
    // point order for bestDist <= TH_LOW (ORBmatcher.cc:1437-1453)
    void FuseCandidates(const orbt_frame &kf, const float Scw[16], const orbt_mappoints &vpPoints, float th,
                        std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist) {
        bestIdx.resize(vpPoints.n);
        bestDist.resize(vpPoints.n);
        check(orbt_fuse_sim3_candidates(track(), &kf, Scw, &vpPoints, th, bestIdx.data(), bestDist.data()),
              "orbt_fuse_sim3_candidates");
    }
    float mfNNratio;
    bool mbCheckOrientation;

private:
    orbm_matcher *handle() {   // created on first use: matchers are cheap stack objects in the reference
        if (!m_) check(orbm_create(mfNNratio, mbCheckOrientation ? 1 : 0, &m_), "orbm_create");
        return m_;
    }
    orbm_matcher *m_ = nullptr;
    static orbb_engine *bow() {
        struct H {
            orbb_engine *h = nullptr;
            H() { check(orbb_create(&h), "orbb_create"); }
            ~H() { orbb_destroy(h); }
        };
        static thread_local H h;
        return h.h;
    }
    static orbt_engine *track() {
        struct H {
            orbt_engine *h = nullptr;
            H() { check(orbt_create(&h), "orbt_create"); }
            ~H() { orbt_destroy(h); }
        };
        static thread_local H h;
        return h.h;
    }
};

// DBoW2 TemplatedVocabulary<FORB::TDescriptor, FORB> (ORBVocabulary.h) resident in HBM.
using BowVector = std::map<uint32_t, double>;                        // DBoW2::BowVector
using FeatureVector = std::map<uint32_t, std::vector<unsigned int>>; // DBoW2::FeatureVector

class ORBVocabulary {
public:
    ORBVocabulary() = default;
    ~ORBVocabulary() { orbv_destroy(h_); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;
    bool loadFromTextFile(const std::string &filename) {
        orbv_destroy(h_);
        h_ = nullptr;
        return orbv_load_text(filename.c_str(), &h_) == ORBX_OK;
    }
    // transform(features, BowVector&, FeatureVector&, levelsup): Frame::ComputeBoW uses 4
    void transform(const uint8_t *desc, int n, BowVector &v, FeatureVector &fv, int levelsup) const {
        v.clear();
        fv.clear();
        std::vector<uint32_t> words(n + 1), nodes(n + 1);
        std::vector<double> vals(n + 1);
        std::vector<int32_t> start(n + 2), feats(n + 1);
        int32_t nw = 0, nf = 0;
        check(orbv_transform(h_, desc, n, levelsup, words.data(), vals.data(), &nw, nodes.data(), start.data(),
                             feats.data(), &nf), "orbv_transform");
        for (int j = 0; j < nw; j++) v.emplace_hint(v.end(), words[j], vals[j]);
        for (int j = 0; j < nf; j++)
            fv.emplace_hint(fv.end(), nodes[j], std::vector<unsigned int>(feats.begin() + start[j], feats.begin() + start[j + 1]));
    }
    size_t size() const {
        int nw = 0;
        if (h_) orbv_info(h_, nullptr, &nw, nullptr, nullptr);
        return (size_t)nw;
    }

private:
    orbv_vocab *h_ = nullptr;
};

// Optimizer::LocalBundleAdjustment minus the map walk: the caller flattens the local
// keyframes / fixed keyframes / local map points / observations into lba_problem
// (Optimizer.cc:646-898 order) and applies the result (SetPose / SetWorldPos /
// EraseMapPointMatch, :977-1048).
struct Sim3KeyFrame;
struct Sim3Match;
struct Sim3;

class Optimizer {
public:
    // Optimizer::OptimizeSim3 (Optimizer.h:186, Optimizer.cc:1405-1637) over the POD views the Sim3Solver
    // takes: vpMatches1[i] is keypoint i of pKF1 (pMP1 = its map point, pMP2 = the match). Edges are added
    // for the entries the reference adds them for (:1471-1512: pMP2 and pMP1 non-NULL, neither bad,
    // indexKF2 >= 0), the whole two-stage optimisation runs on the GPU (orbo_*), removed matches are
    // nulled (pMP2 = false) and g2oS12 is written exactly where the reference writes it: not on the
    // `return 0` of :1605-1606. Returns nIn. Defined below Sim3Solver.
    static int OptimizeSim3(const Sim3KeyFrame &pKF1, const Sim3KeyFrame &pKF2, std::vector<Sim3Match> &vpMatches1,
                            Sim3 &g2oS12, const float th2, const bool bFixScale);
    // The same for every candidate pKF2 of one LoopClosing::ComputeSim3 call in one launch (as
    // Sim3Solver::EvaluateAll): vnInliers[c] = OptimizeSim3(pKF1, *vpKF2[c], *vvpMatches1[c], vg2oS12[c], ..).
    static void OptimizeSim3All(const Sim3KeyFrame &pKF1, const std::vector<const Sim3KeyFrame *> &vpKF2,
                                const std::vector<std::vector<Sim3Match> *> &vvpMatches1, std::vector<Sim3> &vg2oS12,
                                const float th2, const bool bFixScale, std::vector<int> &vnInliers);

    static lba_result LocalBundleAdjustment(const lba_problem &graph, bool *pbStopFlag, std::vector<float> &poseTcw,
                                            std::vector<float> &pointXw, std::vector<uint8_t> &edgeErase) {
        static thread_local LbaHandle lba;
        poseTcw.resize((size_t)graph.n_poses * 16);
        pointXw.resize((size_t)graph.n_points * 3);
        edgeErase.resize(graph.n_edges);
        lba_result r{};
        r.pose_Tcw = poseTcw.data();
        r.point_Xw = pointXw.data();
        r.edge_erase = edgeErase.data();
        static_assert(sizeof(bool) == 1, "pbStopFlag is passed to the C-ABI as one byte");
        check(lba_solve(lba.h, &graph, &r, reinterpret_cast<const volatile uint8_t *>(pbStopFlag)), "lba_solve");
        return r;
    }

    // PoseOptimization(Frame*): edges = the frame's keypoints with a map point, in keypoint
    // order (Optimizer.cc:412-531). Returns nInitialCorrespondences - nBad; Tcw = SetPose
    // value, outlier[k] = mvbOutlier of edge k.
    static int PoseOptimization(const orbp_frame &f, float Tcw[16], std::vector<uint8_t> &outlier) {
        struct H {
            orbp_engine *h = nullptr;
            H() { check(orbp_create(&h), "orbp_create"); }
            ~H() { orbp_destroy(h); }
        };
        static thread_local H eng;
        outlier.assign(f.n, 0);
        orbp_result r{};
        r.outlier = outlier.data();
        check(orbp_pose_optimization(eng.h, &f, &r), "orbp_pose_optimization");
        for (int i = 0; i < 16; i++) Tcw[i] = r.Tcw[i];
        return r.n_inliers;
    }

private:
    struct LbaHandle {
        lba_engine *h = nullptr;
        LbaHandle() { check(lba_create(&h), "lba_create"); }
        ~LbaHandle() { lba_destroy(h); }
    };
};

// LocalMapping::CreateNewMapPoints (LocalMapping.cc:295-600): per neighbour, the caller keeps
// the baseline test, ComputeF12 and ORBmatcher::SearchForTriangulation (orbb_*), then
// TriangulateMatches runs the per-match body on the GPU; ok[k] = 1 -> create the MapPoint at
// x3D[3k..3k+2] with observations (idx1 in mpCurrentKeyFrame, idx2 in pKF2) as the reference does.
class LocalMapping {
public:
    static int TriangulateMatches(const orbn_keyframe &kf1, const orbn_keyframe &kf2,
                                  const std::vector<int32_t> &vMatchedIndices, float ratioFactor,
                                  std::vector<float> &x3D, std::vector<uint8_t> &ok) {
        struct H {
            orbn_engine *h = nullptr;
            H() { check(orbn_create(&h), "orbn_create"); }
            ~H() { orbn_destroy(h); }
        };
        static thread_local H eng;
        const int32_t n = (int32_t)(vMatchedIndices.size() / 2);
        x3D.assign((size_t)n * 3, 0.0f);
        ok.assign(n, 0);
        int32_t nnew = 0;
        check(orbn_triangulate(eng.h, &kf1, &kf2, vMatchedIndices.data(), n, ratioFactor, x3D.data(), ok.data(), &nnew),
              "orbn_triangulate");
        return nnew;
    }
};


// What Sim3Solver's constructor reads of a KeyFrame (Sim3Solver.cc:74-77, 111-112, 138-139).
struct Sim3KeyFrame {
    float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // GetRotation(), row-major
    float tcw[3] = {0, 0, 0};                     // GetTranslation()
    float fx = 0, fy = 0, cx = 0, cy = 0;         // mK
    std::vector<float> mvLevelSigma2;
    std::vector<float> mvInvLevelSigma2;          // Optimizer::OptimizeSim3 (Optimizer.cc:1534, 1556)
};

// Entry i1 of vpMatched12 with everything the constructor dereferences (Sim3Solver.cc:84-135):
// pMP1 = pKF1->GetMapPointMatches()[i1], pMP2 = vpMatched12[i1].
struct Sim3Match {
    bool pMP2 = false, pMP1 = false;      // the pointers are non-NULL
    bool bad1 = false, bad2 = false;      // isBad()
    int indexKF1 = -1, indexKF2 = -1;     // GetIndexInKeyFrame(pKF1 / pKF2)
    int octave1 = 0, octave2 = 0;         // mvKeysUn[indexKF].octave
    float Xw1[3] = {0, 0, 0}, Xw2[3] = {0, 0, 0};   // GetWorldPos()
    // Optimizer::OptimizeSim3 only: pKF1->mvKeysUn[i1].pt and pKF2->mvKeysUn[indexKF2].pt (Optimizer.cc:1522, 1548)
    float pt1[2] = {0, 0}, pt2[2] = {0, 0};
};

// g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h:41-290) as a value type: rotation quaternion (x, y, z, w),
// translation, scale. As in the reference, nothing here normalises the quaternion. With operator*
// the adapter's mg2oScw = gScm * gSmw (LoopClosing.cc:459) needs no g2o.
struct Sim3 {
    double q[4] = {0, 0, 0, 1};
    double t[3] = {0, 0, 0};
    double s = 1.;

    Sim3() {}
    // Sim3(const Quaterniond &r, const Vector3d &t, double s) (sim3.h:59-62); r = (x, y, z, w)
    static Sim3 FromQuaternion(const double r[4], const double t_[3], double s_) {
        Sim3 S;
        for (int k = 0; k < 4; k++) S.q[k] = r[k];
        for (int k = 0; k < 3; k++) S.t[k] = t_[k];
        S.s = s_;
        return S;
    }
    // Sim3(const Matrix3d &R, const Vector3d &t, double s) (sim3.h:64-67): r = Eigen::Quaterniond(R), R row-major
    Sim3(const double R[9], const double t_[3], double s_) : s(s_) {
        for (int k = 0; k < 3; k++) t[k] = t_[k];
        const double *m = R;
        double tr = m[0] + m[4] + m[8];
        if (tr > 0) {
            tr = std::sqrt(tr + 1.0);
            q[3] = 0.5 * tr;
            tr = 0.5 / tr;
            q[0] = (m[7] - m[5]) * tr;
            q[1] = (m[2] - m[6]) * tr;
            q[2] = (m[3] - m[1]) * tr;
        } else {
            int i = 0;
            if (m[4] > m[0]) i = 1;
            if (m[8] > m[4 * i]) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            tr = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
            q[i] = 0.5 * tr;
            tr = 0.5 / tr;
            q[3] = (m[3 * k + j] - m[3 * j + k]) * tr;
            q[j] = (m[3 * j + i] + m[3 * i + j]) * tr;
            q[k] = (m[3 * k + i] + m[3 * i + k]) * tr;
        }
    }

    const double *rotation() const { return q; }      // (x, y, z, w)
    const double *translation() const { return t; }
    double scale() const { return s; }

    // Eigen's Quaternion * Vector3 (_transformVector)
    static void Rotate(const double r[4], const double v[3], double o[3]) {
        double uv[3] = {r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]};
        uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
        const double cx = r[1] * uv[2] - r[2] * uv[1], cy = r[2] * uv[0] - r[0] * uv[2], cz = r[0] * uv[1] - r[1] * uv[0];
        o[0] = v[0] + r[3] * uv[0] + cx;
        o[1] = v[1] + r[3] * uv[1] + cy;
        o[2] = v[2] + r[3] * uv[2] + cz;
    }
    void map(const double xyz[3], double out[3]) const {   // s * (r * xyz) + t
        double p[3];
        Rotate(q, xyz, p);
        for (int k = 0; k < 3; k++) out[k] = s * p[k] + t[k];
    }
    Sim3 inverse() const {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
        Sim3 r;
        r.q[0] = -q[0]; r.q[1] = -q[1]; r.q[2] = -q[2]; r.q[3] = q[3];
        const double f = -1. / s;
        const double v[3] = {f * t[0], f * t[1], f * t[2]};
        Rotate(r.q, v, r.t);
        r.s = 1. / s;
        return r;
    }
    Sim3 operator*(const Sim3 &o) const {
        Sim3 r;
        r.q[3] = q[3] * o.q[3] - q[0] * o.q[0] - q[1] * o.q[1] - q[2] * o.q[2];
        r.q[0] = q[3] * o.q[0] + q[0] * o.q[3] + q[1] * o.q[2] - q[2] * o.q[1];
        r.q[1] = q[3] * o.q[1] + q[1] * o.q[3] + q[2] * o.q[0] - q[0] * o.q[2];
        r.q[2] = q[3] * o.q[2] + q[2] * o.q[3] + q[0] * o.q[1] - q[1] * o.q[0];
        double p[3];
        Rotate(q, o.t, p);
        for (int k = 0; k < 3; k++) r.t[k] = s * p[k] + t[k];
        r.s = s * o.s;
        return r;
    }
};

// Sim3Solver with the reference's members over POD keyframe views. The RANSAC body runs on the GPU:
// the first iterate() (or EvaluateAll over the candidates of one LoopClosing::ComputeSim3 call, one
// launch for all) draws all mRansacMaxIts triplets and evaluates every hypothesis through orbs_*;
// iterate() then replays the reference's loop (Sim3Solver.cc:234-297) over the stored counts, so
// the round-robin of iterate(5) calls (LoopClosing.cc:378-404) costs no launch per call.
// Deviation from the reference: for a given triplet sequence the results are the reference's, but
// the random generator is consumed up front -- 3 * mRansacMaxIts draws per solver -- where the
// reference stops drawing at the early exit, so the process-global rand() stream that later code
// sees is advanced further. RandomInt is injectable (default: DUtils::Random::RandomInt over
// rand(), Thirdparty/DBoW2/DUtils/Random.cpp:47-50) for deterministic runs.
class Sim3Solver {
public:
    using RandomIntFn = std::function<int(int, int)>;

    Sim3Solver(const Sim3KeyFrame &pKF1, const Sim3KeyFrame &pKF2, const std::vector<Sim3Match> &vpMatched12,
               const bool bFixScale = true, RandomIntFn randomInt = RandomIntFn())
        : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale), mRandomInt(randomInt ? randomInt : RandomIntFn(DefaultRandomInt)) {
        mN1 = (int)vpMatched12.size();
        mvnIndices1.reserve(mN1);
        mvX3Dc1.reserve((size_t)mN1 * 3);
        mvX3Dc2.reserve((size_t)mN1 * 3);
        mvAllIndices.reserve(mN1);
        size_t idx = 0;
        for (int i1 = 0; i1 < mN1; i1++) {
            const Sim3Match &m = vpMatched12[i1];
            if (!m.pMP2) continue;
            if (!m.pMP1) continue;
            if (m.bad1 || m.bad2) continue;
            if (m.indexKF1 < 0 || m.indexKF2 < 0) continue;
            const float sigmaSquare1 = pKF1.mvLevelSigma2[m.octave1];
            const float sigmaSquare2 = pKF2.mvLevelSigma2[m.octave2];
            mvnMaxError1.push_back((size_t)(9.210 * sigmaSquare1));   // std::vector<size_t>: truncated (:117-118)
            mvnMaxError2.push_back((size_t)(9.210 * sigmaSquare2));
            mvnIndices1.push_back((size_t)i1);
            ToCamera(pKF1, m.Xw1, mvX3Dc1);
            ToCamera(pKF2, m.Xw2, mvX3Dc2);
            mvAllIndices.push_back(idx);
            idx++;
        }
        mK1[0] = pKF1.fx; mK1[1] = pKF1.fy; mK1[2] = pKF1.cx; mK1[3] = pKF1.cy;
        mK2[0] = pKF2.fx; mK2[1] = pKF2.fy; mK2[2] = pKF2.cx; mK2[3] = pKF2.cy;
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();
        float epsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N)
            nIterations = 1;
        else if (N < mRansacMinInliers)
            nIterations = mRansacMaxIts;   // log of a negative number in the reference; iterate() returns at once
        else
            nIterations = (int)std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
        mEvaluated = false;
    }

    // Evaluates every hypothesis of every solver in one launch (the candidates of one keyframe).
    static void EvaluateAll(std::vector<Sim3Solver *> &vpSolvers) {
        std::vector<Sim3Solver *> todo;
        int capN = 3, capH = 1;
        for (Sim3Solver *s : vpSolvers)
            if (s && !s->mEvaluated && s->N >= s->mRansacMinInliers && s->N >= 3) {
                s->DrawTriplets();
                todo.push_back(s);
                capN = std::max(capN, s->N);
                capH = std::max(capH, s->mRansacMaxIts);
            }
        if (todo.empty()) return;
        Engine &eng = engine();
        check(orbs_reserve(eng.h, (int)todo.size(), capN, capH), "orbs_reserve");
        for (size_t k = 0; k < todo.size(); k++) {
            orbs_problem p = todo[k]->Problem();
            check(orbs_stage(eng.h, (int)k, &p), "orbs_stage");
        }
        check(orbs_run_batch(eng.h, (int)todo.size(), nullptr), "orbs_run_batch");
        for (size_t k = 0; k < todo.size(); k++) {
            orbs_result r = todo[k]->Result();
            check(orbs_fetch(eng.h, (int)k, &r), "orbs_fetch");
            todo[k]->mEvaluated = true;
        }
    }

    // Returns true where the reference returns a non-empty mBestT12 (T12 = [s R | t; 0 1], row-major).
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float T12[16] = nullptr) {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers || N < 3) {   // N < 3: no min set can be drawn (the reference would index out of range)
            bNoMore = true;
            return false;
        }
        if (!mEvaluated) {
            std::vector<Sim3Solver *> self{this};
            EvaluateAll(self);
        }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int h = mnIterations++;
            const int mnInliersi = mvnInliers[h];
            if (mnInliersi >= mnBestInliers) {
                mnBestInliers = mnInliersi;
                mnBest = h;
                if (mnInliersi > mRansacMinInliers) {
                    nInliers = mnInliersi;
                    const size_t w = ((size_t)N + 63) / 64;
                    for (int i = 0; i < N; i++)
                        if ((mvInlierBits[(size_t)h * w + i / 64] >> (i % 64)) & 1) vbInliers[mvnIndices1[i]] = true;
                    if (T12) {
                        const float s = mvScale[h];
                        for (int r = 0; r < 3; r++) {
                            for (int c = 0; c < 3; c++) T12[4 * r + c] = s * mvRotation[(size_t)h * 9 + 3 * r + c];
                            T12[4 * r + 3] = mvTranslation[(size_t)h * 3 + r];
                        }
                        T12[12] = T12[13] = T12[14] = 0;
                        T12[15] = 1;
                    }
                    return true;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return false;
    }

    bool find(std::vector<bool> &vbInliers12, int &nInliers, float T12[16] = nullptr) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
    }

    // mBestRotation (row-major 3x3) / mBestTranslation / mBestScale; false before any iteration
    bool GetEstimatedRotation(float R[9]) const {
        if (mnBest < 0) return false;
        for (int k = 0; k < 9; k++) R[k] = mvRotation[(size_t)mnBest * 9 + k];
        return true;
    }
    bool GetEstimatedTranslation(float t[3]) const {
        if (mnBest < 0) return false;
        for (int k = 0; k < 3; k++) t[k] = mvTranslation[(size_t)mnBest * 3 + k];
        return true;
    }
    float GetEstimatedScale() const { return mnBest < 0 ? 0.0f : mvScale[mnBest]; }

    int GetNumCorrespondences() const { return N; }          // N
    int GetMaxIterations() const { return mRansacMaxIts; }   // mRansacMaxIts after SetRansacParameters
    int GetIterations() const { return mnIterations; }       // mnIterations
    const std::vector<size_t> &GetMaxError1() const { return mvnMaxError1; }
    const std::vector<int32_t> &GetTriplets() const { return mvTriplets; }

    static int DefaultRandomInt(int min, int max) {   // DUtils::Random::RandomInt
        int d = max - min + 1;
        return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
    }

private:
    friend class Optimizer;   // OptimizeSim3 computes P3D1c / P3D2c with ToCamera
    struct Engine {
        orbs_engine *h = nullptr;
        Engine() { check(orbs_create(&h), "orbs_create"); }
        ~Engine() { orbs_destroy(h); }
    };
    static Engine &engine() {
        static thread_local Engine eng;
        return eng;
    }

    static void ToCamera(const Sim3KeyFrame &kf, const float Xw[3], std::vector<float> &out) {   // Rcw * X3Dw + tcw, float
        for (int r = 0; r < 3; r++) {
            float s = kf.Rcw[3 * r] * Xw[0];
            s = s + kf.Rcw[3 * r + 1] * Xw[1];
            s = s + kf.Rcw[3 * r + 2] * Xw[2];
            out.push_back(s + kf.tcw[r]);
        }
    }

    // the min sets of all mRansacMaxIts iterations, drawn as the reference's loop does (:240-261)
    void DrawTriplets() {
        mvTriplets.clear();
        mvTriplets.reserve((size_t)mRansacMaxIts * 3);
        std::vector<size_t> vAvailableIndices;
        for (int it = 0; it < mRansacMaxIts; it++) {
            vAvailableIndices = mvAllIndices;
            for (short i = 0; i < 3; ++i) {
                int randi = mRandomInt(0, (int)vAvailableIndices.size() - 1);
                mvTriplets.push_back((int32_t)vAvailableIndices[randi]);
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
    }

    orbs_problem Problem() {
        mvMaxErrorF1.resize(N);
        mvMaxErrorF2.resize(N);
        for (int i = 0; i < N; i++) {   // err < mvnMaxError[i]: the size_t converted to float (:480)
            mvMaxErrorF1[i] = (float)mvnMaxError1[i];
            mvMaxErrorF2[i] = (float)mvnMaxError2[i];
        }
        orbs_problem p{};
        p.n = N;
        p.X1c = mvX3Dc1.data();
        p.X2c = mvX3Dc2.data();
        p.max_err1 = mvMaxErrorF1.data();
        p.max_err2 = mvMaxErrorF2.data();
        for (int k = 0; k < 4; k++) {
            p.K1[k] = mK1[k];
            p.K2[k] = mK2[k];
        }
        p.fix_scale = mbFixScale ? 1 : 0;
        p.n_hyp = mRansacMaxIts;
        p.triplets = mvTriplets.data();
        return p;
    }

    orbs_result Result() {
        const size_t H = (size_t)mRansacMaxIts, w = ((size_t)N + 63) / 64;
        mvnInliers.assign(H, 0);
        mvInlierBits.assign(H * w, 0);
        mvRotation.assign(H * 9, 0.0f);
        mvTranslation.assign(H * 3, 0.0f);
        mvScale.assign(H, 0.0f);
        return orbs_result{mvnInliers.data(), mvInlierBits.data(), mvRotation.data(), mvTranslation.data(), mvScale.data()};
    }

    int mN1 = 0, N = 0;
    std::vector<size_t> mvnIndices1, mvnMaxError1, mvnMaxError2, mvAllIndices;
    std::vector<float> mvX3Dc1, mvX3Dc2, mvMaxErrorF1, mvMaxErrorF2;
    float mK1[4], mK2[4];
    int mnIterations, mnBestInliers, mnBest = -1;
    bool mbFixScale, mEvaluated = false;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    RandomIntFn mRandomInt;
    std::vector<int32_t> mvTriplets, mvnInliers;
    std::vector<uint64_t> mvInlierBits;
    std::vector<float> mvRotation, mvTranslation, mvScale;
};

namespace detail {
// the edges of one OptimizeSim3 call (Optimizer.cc:1469-1566), compacted in vnIndexEdge order
struct Sim3OptGraph {
    std::vector<size_t> vnIndexEdge;
    std::vector<float> X1c, X2c, obs1, obs2, inv1, inv2;
    std::vector<uint8_t> state;
    orbo_problem Problem(const Sim3KeyFrame &pKF1, const Sim3KeyFrame &pKF2, const Sim3 &g2oS12, float th2, bool bFixScale) {
        orbo_problem p{};
        p.n = (int32_t)vnIndexEdge.size();
        p.X1c = X1c.data(); p.X2c = X2c.data();
        p.obs1 = obs1.data(); p.obs2 = obs2.data();
        p.inv_sigma2_1 = inv1.data(); p.inv_sigma2_2 = inv2.data();
        p.K1[0] = pKF1.fx; p.K1[1] = pKF1.fy; p.K1[2] = pKF1.cx; p.K1[3] = pKF1.cy;
        p.K2[0] = pKF2.fx; p.K2[1] = pKF2.fy; p.K2[2] = pKF2.cx; p.K2[3] = pKF2.cy;
        for (int k = 0; k < 4; k++) p.q[k] = g2oS12.q[k];
        for (int k = 0; k < 3; k++) p.t[k] = g2oS12.t[k];
        p.s = g2oS12.s;
        p.th2 = th2;
        p.fix_scale = bFixScale ? 1 : 0;
        return p;
    }
};
struct Sim3OptEngine {
    orbo_engine *h = nullptr;
    Sim3OptEngine() { check(orbo_create(&h), "orbo_create"); }
    ~Sim3OptEngine() { orbo_destroy(h); }
};
}  // namespace detail

inline void Optimizer::OptimizeSim3All(const Sim3KeyFrame &pKF1, const std::vector<const Sim3KeyFrame *> &vpKF2,
                                       const std::vector<std::vector<Sim3Match> *> &vvpMatches1, std::vector<Sim3> &vg2oS12,
                                       const float th2, const bool bFixScale, std::vector<int> &vnInliers) {
    static thread_local detail::Sim3OptEngine eng;
    const size_t nc = vpKF2.size();
    if (vvpMatches1.size() != nc || vg2oS12.size() != nc) throw std::runtime_error("OptimizeSim3All: size mismatch");
    vnInliers.assign(nc, 0);
    if (!nc) return;
    std::vector<detail::Sim3OptGraph> graphs(nc);
    int cap = 0;
    for (size_t c = 0; c < nc; c++) {
        detail::Sim3OptGraph &g = graphs[c];
        const Sim3KeyFrame &pKF2 = *vpKF2[c];
        const std::vector<Sim3Match> &vpMatches1 = *vvpMatches1[c];
        const int N = (int)vpMatches1.size();
        for (int i = 0; i < N; i++) {
            const Sim3Match &m = vpMatches1[i];
            if (!m.pMP2) continue;                                // :1471
            if (!m.pMP1) continue;                                // :1485, 1511
            if (m.bad1 || m.bad2 || m.indexKF2 < 0) continue;     // :1487, 1508
            Sim3Solver::ToCamera(pKF1, m.Xw1, g.X1c);             // P3D1c = R1w * P3D1w + t1w
            Sim3Solver::ToCamera(pKF2, m.Xw2, g.X2c);
            g.obs1.push_back(m.pt1[0]); g.obs1.push_back(m.pt1[1]);
            g.obs2.push_back(m.pt2[0]); g.obs2.push_back(m.pt2[1]);
            g.inv1.push_back(pKF1.mvInvLevelSigma2[m.octave1]);
            g.inv2.push_back(pKF2.mvInvLevelSigma2[m.octave2]);
            g.vnIndexEdge.push_back((size_t)i);
        }
        cap = std::max(cap, (int)g.vnIndexEdge.size());
    }
    check(orbo_reserve(eng.h, (int)nc, cap), "orbo_reserve");
    for (size_t c = 0; c < nc; c++) {
        const orbo_problem p = graphs[c].Problem(pKF1, *vpKF2[c], vg2oS12[c], th2, bFixScale);
        check(orbo_stage(eng.h, (int)c, &p), "orbo_stage");
    }
    check(orbo_run_batch(eng.h, (int)nc, nullptr), "orbo_run_batch");
    for (size_t c = 0; c < nc; c++) {
        detail::Sim3OptGraph &g = graphs[c];
        g.state.assign(std::max<size_t>(g.vnIndexEdge.size(), 1), 0);
        orbo_result r{};
        r.state = g.state.data();
        check(orbo_fetch(eng.h, (int)c, &r), "orbo_fetch");
        for (size_t k = 0; k < g.vnIndexEdge.size(); k++)
            if (g.state[k]) (*vvpMatches1[c])[g.vnIndexEdge[k]].pMP2 = false;   // vpMatches1[idx] = NULL (:1587, 1625)
        if (r.iterations[1] >= 0)                                               // past the `return 0` of :1605-1606
            vg2oS12[c] = Sim3::FromQuaternion(r.q, r.t, r.s);                            // g2oS12 = vSim3_recov->estimate()
        vnInliers[c] = r.n_inliers;
    }
}

inline int Optimizer::OptimizeSim3(const Sim3KeyFrame &pKF1, const Sim3KeyFrame &pKF2, std::vector<Sim3Match> &vpMatches1,
                                   Sim3 &g2oS12, const float th2, const bool bFixScale) {
    std::vector<const Sim3KeyFrame *> vpKF2{&pKF2};
    std::vector<std::vector<Sim3Match> *> vvp{&vpMatches1};
    std::vector<Sim3> vS{g2oS12};
    std::vector<int> vn;
    OptimizeSim3All(pKF1, vpKF2, vvp, vS, th2, bFixScale, vn);
    g2oS12 = vS[0];
    return vn[0];
}

// ---- KeyFrameDatabase (orbd_*) and LoopClosing::DetectLoop -------------------------------------------------

// What KeyFrameDatabase and LoopClosing::DetectLoop read of a KeyFrame. Keyframes are named by mnId.
struct KeyFrameView {
    int64_t mnId = 0;
    BowVector mBowVec;
    std::vector<int64_t> connected;    // GetConnectedKeyFrames(): every keyframe sharing a map point
    std::vector<int64_t> covisibles;   // GetVectorCovisibleKeyFrames(): mvpOrderedConnectedKeyFrames without the bad
                                       // ones; its first 10 are GetBestCovisibilityKeyFrames(10)
};

struct FrameView {                     // what DetectRelocalizationCandidates reads of a Frame
    BowVector mBowVec;
};

class KeyFrameDatabase {
public:
    // KeyFrameDatabase(const ORBVocabulary &voc): one inverted list per word (KeyFrameDatabase.cc:45-50)
    explicit KeyFrameDatabase(const ORBVocabulary &voc) : KeyFrameDatabase(voc.size()) {}
    explicit KeyFrameDatabase(size_t n_words) { check(orbd_create((int)n_words, ORBD_L1_NORM, &h_), "orbd_create"); }
    ~KeyFrameDatabase() { orbd_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    // add(pKF): the BowVector goes to HBM with the keyframe's 10 best covisibles (the group walk of both
    // queries reads pKFi->GetBestCovisibilityKeyFrames(10) of database keyframes)
    void add(const KeyFrameView &kf) {
        flatten(kf.mBowVec);
        check(orbd_add(h_, kf.mnId, w_.data(), v_.data(), (int)w_.size()), "orbd_add");
        SetCovisibles(kf.mnId, kf.covisibles);
    }
    // the covisibility graph changed (KeyFrame::UpdateConnections / UpdateBestCovisibles) for a stored keyframe
    void SetCovisibles(int64_t mnId, const std::vector<int64_t> &ordered) {
        const int n = (int)std::min<size_t>(ordered.size(), ORBD_MAX_COVISIBLES);
        check(orbd_set_covisibles(h_, mnId, ordered.data(), n), "orbd_set_covisibles");
    }
    void erase(int64_t mnId) { check(orbd_erase(h_, mnId), "orbd_erase"); }
    void clear() { check(orbd_clear(h_), "orbd_clear"); }
    size_t size() const {
        int32_t n = 0;
        check(orbd_size(h_, &n), "orbd_size");
        return (size_t)n;
    }

    // vector<KeyFrame*> DetectLoopCandidates(KeyFrame *pKF, float minScore) (KeyFrameDatabase.cc:113-264)
    std::vector<int64_t> DetectLoopCandidates(const KeyFrameView &kf, float minScore) {
        return detect(ORBD_LOOP, kf.mBowVec, &kf.connected, minScore);
    }
    // vector<KeyFrame*> DetectRelocalizationCandidates(Frame *F) (:275-418)
    std::vector<int64_t> DetectRelocalizationCandidates(const FrameView &F) { return detect(ORBD_RELOC, F.mBowVec, nullptr, 0.0f); }
    // The covisible scan of LoopClosing::DetectLoop (LoopClosing.cc:163-184): the smallest
    // mpORBVocabulary->score(bow, keyframe) over `ids`, starting at 1; keyframes that are not in the database
    // (bad ones were erased) are skipped. scores (may be NULL) gets one float per id, -1 = skipped.
    float Scores(const BowVector &bow, const std::vector<int64_t> &ids, std::vector<float> *scores = nullptr) {
        flatten(bow);
        std::vector<float> sc(ids.size() + 1);
        float min_score = 1.0f;
        check(orbd_scores(h_, w_.data(), v_.data(), (int)w_.size(), ids.data(), (int)ids.size(), sc.data(), &min_score),
              "orbd_scores");
        sc.resize(ids.size());
        if (scores) *scores = sc;
        return min_score;
    }
    orbd_db *handle() { return h_; }

private:
    void flatten(const BowVector &b) {
        w_.clear();
        v_.clear();
        for (const auto &e : b) {
            w_.push_back(e.first);
            v_.push_back(e.second);
        }
        if (w_.empty()) {   // non-NULL pointers for an empty vector
            w_.reserve(1);
            v_.reserve(1);
        }
    }
    std::vector<int64_t> detect(int kind, const BowVector &bow, const std::vector<int64_t> *connected, float minScore) {
        flatten(bow);
        orbd_query q{};
        q.kind = kind;
        q.n = (int32_t)w_.size();
        q.words = w_.data();
        q.values = v_.data();
        q.connected = connected && !connected->empty() ? connected->data() : nullptr;
        q.n_connected = connected ? (int32_t)connected->size() : 0;
        q.min_score = minScore;
        std::vector<int64_t> cand(size() + 1);
        orbd_result r{};
        r.cap = (int32_t)cand.size();
        r.candidates = cand.data();
        check(orbd_detect(h_, &q, &r), "orbd_detect");
        cand.resize((size_t)r.n_candidates);
        return cand;
    }
    orbd_db *h_ = nullptr;
    std::vector<uint32_t> w_;
    std::vector<double> v_;
};

// LoopClosing::DetectLoop (LoopClosing.cc:137-285) over a database DB with Scores / DetectLoopCandidates / add
// (orbslam2_amd::KeyFrameDatabase, or a stand-in). The queue, SetNotErase / SetErase and the map stay with the
// caller; connected_of(id) is pCandidateKF->GetConnectedKeyFrames() of a candidate.
template <class DB>
class LoopClosingT {
public:
    typedef std::pair<std::set<int64_t>, int> ConsistentGroup;
    LoopClosingT(DB *pDB, std::function<std::vector<int64_t>(int64_t)> connected_of)
        : mpKeyFrameDB(pDB), connected_of_(std::move(connected_of)) {}

    bool DetectLoop(const KeyFrameView &currentKF) {
        // :152 less than 10 keyframes since the last loop
        if (currentKF.mnId < mLastLoopKFid + 10) {
            mpKeyFrameDB->add(currentKF);
            return false;
        }
        // :163-178 the lowest score to a connected keyframe of the covisibility graph
        const float minScore = mpKeyFrameDB->Scores(currentKF.mBowVec, currentKF.covisibles);
        mLastMinScore = minScore;
        // :184
        const std::vector<int64_t> vpCandidateKFs = mpKeyFrameDB->DetectLoopCandidates(currentKF, minScore);
        if (vpCandidateKFs.empty()) {   // :188-194
            mpKeyFrameDB->add(currentKF);
            mvConsistentGroups.clear();
            return false;
        }
        // :202-268 a candidate's group is consistent with a previous group if they share a keyframe
        mvpEnoughConsistentCandidates.clear();
        std::vector<ConsistentGroup> vCurrentConsistentGroups;
        std::vector<bool> vbConsistentGroup(mvConsistentGroups.size(), false);
        for (size_t i = 0, iend = vpCandidateKFs.size(); i < iend; i++) {
            const int64_t pCandidateKF = vpCandidateKFs[i];
            const std::vector<int64_t> conn = connected_of_(pCandidateKF);
            std::set<int64_t> spCandidateGroup(conn.begin(), conn.end());
            spCandidateGroup.insert(pCandidateKF);
            bool bEnoughConsistent = false;
            bool bConsistentForSomeGroup = false;
            for (size_t iG = 0, iendG = mvConsistentGroups.size(); iG < iendG; iG++) {
                const std::set<int64_t> &sPreviousGroup = mvConsistentGroups[iG].first;
                bool bConsistent = false;
                for (std::set<int64_t>::const_iterator sit = spCandidateGroup.begin(), send = spCandidateGroup.end(); sit != send; sit++) {
                    if (sPreviousGroup.count(*sit)) {
                        bConsistent = true;
                        bConsistentForSomeGroup = true;
                        break;
                    }
                }
                if (bConsistent) {
                    const int nCurrentConsistency = mvConsistentGroups[iG].second + 1;
                    if (!vbConsistentGroup[iG]) {
                        vCurrentConsistentGroups.push_back(std::make_pair(spCandidateGroup, nCurrentConsistency));
                        vbConsistentGroup[iG] = true;
                    }
                    if (nCurrentConsistency >= mnCovisibilityConsistencyTh && !bEnoughConsistent) {
                        mvpEnoughConsistentCandidates.push_back(pCandidateKF);
                        bEnoughConsistent = true;
                    }
                }
            }
            if (!bConsistentForSomeGroup) vCurrentConsistentGroups.push_back(std::make_pair(spCandidateGroup, 0));
        }
        mvConsistentGroups = vCurrentConsistentGroups;   // :272
        mpKeyFrameDB->add(currentKF);                    // :274
        return !mvpEnoughConsistentCandidates.empty();
    }

    int64_t mLastLoopKFid = 0;                 // set by the caller's CorrectLoop (LoopClosing.cc:785)
    int mnCovisibilityConsistencyTh = 3;       // LoopClosing.cc:56
    std::vector<ConsistentGroup> mvConsistentGroups;
    std::vector<int64_t> mvpEnoughConsistentCandidates;
    float mLastMinScore = 1.0f;                // the minScore of the last call that reached the query

private:
    DB *mpKeyFrameDB;
    std::function<std::vector<int64_t>(int64_t)> connected_of_;
};
using LoopClosing = LoopClosingT<KeyFrameDatabase>;

}  // namespace orbslam2_amd
