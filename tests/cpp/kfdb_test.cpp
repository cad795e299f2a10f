// Driver of orbslam2_amd::KeyFrameDatabase and LoopClosing::DetectLoop (host/orbslam2_amd.hpp).
//   kfdb_test stub <script> <out>   DetectLoop over a stand-in database whose candidates and minimum scores
//                                   come from a table: the consistency-group bookkeeping alone, no device
//   kfdb_test mincw <max> <out>    int minCommonWords = maxCommonWords * 0.8f (KeyFrameDatabase.cc:174) for 1..max
//   kfdb_test gpu <problem> <out>   the real database: add / SetCovisibles / erase, both queries and Scores
// Inputs and outputs are whitespace-separated text; doubles and floats travel as C99 hex literals.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "orbslam2_amd.hpp"

using namespace orbslam2_amd;

static long long rd_int(std::istream &in) {
    long long v = 0;
    in >> v;
    return v;
}
static double rd_hex(std::istream &in) {
    std::string s;
    in >> s;
    return std::strtod(s.c_str(), nullptr);
}
static std::vector<int64_t> rd_ids(std::istream &in) {
    std::vector<int64_t> v((size_t)rd_int(in));
    for (auto &x : v) x = rd_int(in);
    return v;
}
static BowVector rd_bow(std::istream &in) {
    const int n = (int)rd_int(in);
    std::vector<uint32_t> w(n);
    for (auto &x : w) x = (uint32_t)rd_int(in);
    BowVector b;
    for (int i = 0; i < n; i++) b.emplace_hint(b.end(), w[i], rd_hex(in));
    return b;
}

// The stand-in: candidates and the covisible minimum score by keyframe id, every call logged
struct TableDB {
    std::map<int64_t, std::vector<int64_t>> candidates;
    std::map<int64_t, float> min_score;
    std::vector<int64_t> added;
    int64_t scoring = -1;
    std::vector<float> seen_min_scores;
    void add(const KeyFrameView &kf) { added.push_back(kf.mnId); }
    float Scores(const BowVector &, const std::vector<int64_t> &ids) {
        scoring = ids.empty() ? -1 : ids[0];   // the script puts the keyframe's own id first in its covisibles
        return min_score.count(scoring) ? min_score[scoring] : 1.0f;
    }
    std::vector<int64_t> DetectLoopCandidates(const KeyFrameView &kf, float minScore) {
        seen_min_scores.push_back(minScore);
        return candidates[kf.mnId];
    }
};

static int run_stub(const char *script, const char *out_path) {
    std::ifstream in(script);
    if (!in) return 2;
    TableDB db;
    std::map<int64_t, std::vector<int64_t>> connected;
    const int n_conn = (int)rd_int(in);
    for (int i = 0; i < n_conn; i++) {
        const int64_t id = rd_int(in);
        connected[id] = rd_ids(in);
    }
    const int n_steps = (int)rd_int(in);
    LoopClosingT<TableDB> lc(&db, [&](int64_t id) { return connected[id]; });
    FILE *out = std::fopen(out_path, "w");
    if (!out) return 2;
    for (int s = 0; s < n_steps; s++) {
        KeyFrameView kf;
        kf.mnId = rd_int(in);
        kf.covisibles = {kf.mnId};
        db.min_score[kf.mnId] = (float)rd_hex(in);
        db.candidates[kf.mnId] = rd_ids(in);
        const long long last = rd_int(in);   // >= 0: CorrectLoop ran before this keyframe and set mLastLoopKFid
        if (last >= 0) lc.mLastLoopKFid = last;
        const size_t queries = db.seen_min_scores.size();
        const bool loop = lc.DetectLoop(kf);
        std::fprintf(out, "%lld %d enough", (long long)kf.mnId, loop ? 1 : 0);
        for (int64_t c : lc.mvpEnoughConsistentCandidates) std::fprintf(out, " %lld", (long long)c);
        std::fprintf(out, " groups");
        for (const auto &g : lc.mvConsistentGroups) {
            std::fprintf(out, " %d:", g.second);
            for (int64_t m : g.first) std::fprintf(out, "%lld,", (long long)m);
        }
        if (db.seen_min_scores.size() > queries) std::fprintf(out, " minScore %a", (double)db.seen_min_scores.back());
        std::fprintf(out, " added %zu\n", db.added.size());
    }
    std::fclose(out);
    return 0;
}

static int run_gpu(const char *problem, const char *out_path) {
    std::ifstream in(problem);
    if (!in) return 2;
    const size_t n_words = (size_t)rd_int(in);
    KeyFrameDatabase db(n_words);
    FILE *out = std::fopen(out_path, "w");
    if (!out) return 2;
    std::string op;
    while (in >> op) {
        if (op == "add") {
            KeyFrameView kf;
            kf.mnId = rd_int(in);
            kf.mBowVec = rd_bow(in);
            kf.covisibles = rd_ids(in);
            db.add(kf);
        } else if (op == "cov") {
            const int64_t id = rd_int(in);
            db.SetCovisibles(id, rd_ids(in));
        } else if (op == "erase") {
            db.erase(rd_int(in));
        } else if (op == "clear") {
            db.clear();
        } else if (op == "loop" || op == "reloc") {
            std::vector<int64_t> cand;
            if (op == "loop") {
                KeyFrameView kf;
                kf.mBowVec = rd_bow(in);
                kf.connected = rd_ids(in);
                const float min_score = (float)rd_hex(in);
                cand = db.DetectLoopCandidates(kf, min_score);
            } else {
                FrameView F;
                F.mBowVec = rd_bow(in);
                cand = db.DetectRelocalizationCandidates(F);
            }
            std::fprintf(out, "%s", op.c_str());
            for (int64_t c : cand) std::fprintf(out, " %lld", (long long)c);
            std::fprintf(out, "\n");
        } else if (op == "scores") {
            const BowVector b = rd_bow(in);
            const std::vector<int64_t> ids = rd_ids(in);
            std::vector<float> sc;
            const float mn = db.Scores(b, ids, &sc);
            std::fprintf(out, "scores %a", (double)mn);
            for (float s : sc) std::fprintf(out, " %a", (double)s);
            std::fprintf(out, "\n");
        } else if (op == "size") {
            std::fprintf(out, "size %zu\n", db.size());
        } else {
            return 3;
        }
    }
    std::fclose(out);
    return 0;
}

static int run_mincw(int max, const char *out_path) {
    FILE *out = std::fopen(out_path, "w");
    if (!out) return 2;
    for (volatile int maxCommonWords = 1; maxCommonWords <= max; maxCommonWords = maxCommonWords + 1) {
        int minCommonWords = maxCommonWords * 0.8f;
        std::fprintf(out, "%d\n", minCommonWords);
    }
    std::fclose(out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 1;
    try {
        if (std::string(argv[1]) == "mincw") return run_mincw(std::atoi(argv[2]), argv[3]);
        if (std::string(argv[1]) == "stub") return run_stub(argv[2], argv[3]);
        if (std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    return 1;
}
