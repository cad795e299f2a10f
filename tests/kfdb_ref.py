"""KeyFrameDatabase restated on the CPU, statement by statement (KeyFrameDatabase.cc:57-418), with the
containers shaped like the reference's: mvInvertedFile is a list (one entry per word) of lists of
keyframes, and every keyframe carries mnLoopQuery / mnLoopWords / mLoopScore / mnRelocQuery /
mnRelocWords / mRelocScore. L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) is a
Python-float (IEEE double) sum, one rounding per operation. float members are numpy float32.

Pins: every query gets a fresh id (never 0, never repeated); mRelocScore, which the reference leaves
uninitialised, starts at 0.0f; a neighbour id that is not in the database is skipped.

brute_force() is the second formulation the GPU library uses (shared words = set intersection, list
order = (first common word, add sequence)); tests/test_kfdb_cpu.py checks the two agree."""
import bisect

import numpy as np

F32 = np.float32
LOOP, RELOC = 0, 1


class KF:
    def __init__(self, mnId, words, values):
        self.mnId = int(mnId)
        self.words = [int(w) for w in words]            # mBowVec: std::map<WordId, WordValue>, ascending
        self.values = [float(v) for v in values]
        self.covisibles = []                            # mvpOrderedConnectedKeyFrames[0..10) as ids
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = F32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)                       # pinned: uninitialised in the reference


def score(w1, v1, w2, v2):
    """L1Scoring::score(v1, v2), then the float the callers store it in."""
    i = j = 0
    n1, n2 = len(w1), len(w2)
    s = 0.0
    while i < n1 and j < n2:
        if w1[i] == w2[j]:
            vi, wi = v1[i], v2[j]
            s += (abs(vi - wi) - abs(vi)) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j], i)        # v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(w2, w1[i], j)
    s = -s / 2.0
    return F32(s)


def min_common_words(m):
    """int minCommonWords = maxCommonWords * 0.8f"""
    return int(F32(m) * F32(0.8))


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.kfs = {}
        self.next_query = 1

    def add(self, mnId, words, values):
        assert mnId not in self.kfs
        kf = KF(mnId, words, values)
        self.kfs[kf.mnId] = kf
        for w in kf.words:
            self.mvInvertedFile[w].append(kf)
        return kf

    def erase(self, mnId):
        kf = self.kfs.pop(mnId)
        for w in kf.words:
            lKFs = self.mvInvertedFile[w]
            for k, other in enumerate(lKFs):
                if other is kf:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = [[] for _ in range(self.n_words)]
        self.kfs = {}

    def set_covisibles(self, mnId, ids):
        assert len(ids) <= 10
        self.kfs[mnId].covisibles = [int(i) for i in ids]

    def _neighbours(self, kf):
        """GetBestCovisibilityKeyFrames(10); an id that is not in the database is skipped"""
        return [self.kfs[i] for i in kf.covisibles[:10] if i in self.kfs]

    @staticmethod
    def _result(lScoreAndMatch=(), lAcc=(), cands=(), maxc=0, minc=0):
        return {"candidates": np.array([k.mnId for k in cands], np.int64),
                "scored_ids": np.array([k.mnId for _, k in lScoreAndMatch], np.int64),
                "scored_si": np.array([s for s, _ in lScoreAndMatch], np.float32),
                "scored_words": np.array([k._words_now for _, k in lScoreAndMatch], np.int32),
                "acc_score": np.array([a for a, _ in lAcc], np.float32),
                "acc_best": np.array([k.mnId for _, k in lAcc], np.int64),
                "max_common_words": maxc, "min_common_words": minc}

    def DetectLoopCandidates(self, words, values, connected, minScore):
        minScore = F32(minScore)
        qid = self.next_query
        self.next_query += 1
        spConnectedKeyFrames = {self.kfs[i] for i in connected if i in self.kfs}
        lKFsSharingWords = []
        for w in words:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != qid:
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = qid
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        if not lKFsSharingWords:
            return self._result()
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = min_common_words(maxCommonWords)
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = score(words, values, pKFi.words, pKFi.values)
                pKFi.mLoopScore = si
                pKFi._words_now = pKFi.mnLoopWords
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return self._result(maxc=maxCommonWords, minc=minCommonWords)
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnLoopQuery == qid and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lScoreAndMatch, lAccScoreAndMatch, bestAccScore, maxCommonWords, minCommonWords)

    def DetectRelocalizationCandidates(self, words, values):
        qid = self.next_query
        self.next_query += 1
        lKFsSharingWords = []
        for w in words:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != qid:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = qid
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return self._result()
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = min_common_words(maxCommonWords)
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = score(words, values, pKFi.words, pKFi.values)
                pKFi.mRelocScore = si
                pKFi._words_now = pKFi.mnRelocWords
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return self._result(maxc=maxCommonWords, minc=minCommonWords)
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnRelocQuery != qid:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)     # stale where pKF2 failed the word threshold
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lScoreAndMatch, lAccScoreAndMatch, bestAccScore, maxCommonWords, minCommonWords)

    def _retain(self, lScoreAndMatch, lAccScoreAndMatch, bestAccScore, maxc, minc):
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpCandidates = []
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if pKFi not in spAlreadyAddedKF:
                    vpCandidates.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        return self._result(lScoreAndMatch, lAccScoreAndMatch, vpCandidates, maxc, minc)

    def query(self, q):
        if q["kind"] == LOOP:
            return self.DetectLoopCandidates(q["words"], q["values"], q.get("connected", ()), q["min_score"])
        return self.DetectRelocalizationCandidates(q["words"], q["values"])

    def scores(self, words, values, ids):
        """LoopClosing::DetectLoop's covisible scan (LoopClosing.cc:163-184); -1 = not in the database"""
        minScore = F32(1)
        out = np.full(len(ids), -1, np.float32)
        for k, i in enumerate(ids):
            if i not in self.kfs:
                continue
            kf = self.kfs[i]
            s = score(words, values, kf.words, kf.values)
            out[k] = s
            if s < minScore:
                minScore = s
        return out, minScore

    # ---- the formulation the GPU library uses ----
    def brute_force(self, words, connected=()):
        """(ids of lKFsSharingWords in list order, their shared-word counts) from set intersections and
        add sequence numbers. The sequence of a keyframe = the position of its last add."""
        seq = {kf.mnId: n for n, kf in enumerate(self.kfs.values())}    # dict order = add order; erase + add re-inserts
        qs = set(words)
        rows = []
        for kf in self.kfs.values():
            if kf.mnId in connected:
                continue
            common = qs.intersection(kf.words)
            if common:
                rows.append((min(common), seq[kf.mnId], kf.mnId, len(common)))
        rows.sort()
        return [r[2] for r in rows], [r[3] for r in rows]

    def sharing_words(self, words, connected=()):
        """lKFsSharingWords and the counts by the reference's inverted-file walk (no state kept)"""
        seen, order = {}, []
        conn = set(connected)
        for w in words:
            for kf in self.mvInvertedFile[w]:
                if kf.mnId in conn:
                    continue
                if kf.mnId not in seen:
                    seen[kf.mnId] = 0
                    order.append(kf.mnId)
                seen[kf.mnId] += 1
        return order, [seen[i] for i in order]


# ---- LoopClosing::DetectLoop (LoopClosing.cc:137-285) over a scripted candidate source ----
class DetectLoopRef:
    """The consistency-group bookkeeping: `candidates(kf_id)` stands in for DetectLoopCandidates,
    `connected(kf_id)` for GetConnectedKeyFrames. Returns (loop?, mvpEnoughConsistentCandidates); the member is
    cleared at :202 only, so the early returns leave the previous call's list in place, as the reference does."""

    def __init__(self, candidates, connected):
        self.candidates, self.connected = candidates, connected
        self.mLastLoopKFid = 0
        self.mvConsistentGroups = []
        self.mvpEnoughConsistentCandidates = []
        self.added = []

    def DetectLoop(self, mnId):
        if mnId < self.mLastLoopKFid + 10:
            self.added.append(mnId)
            return False, list(self.mvpEnoughConsistentCandidates)
        vpCandidateKFs = self.candidates(mnId)
        if not vpCandidateKFs:
            self.added.append(mnId)
            self.mvConsistentGroups = []
            return False, list(self.mvpEnoughConsistentCandidates)
        enough = self.mvpEnoughConsistentCandidates = []
        vCurrentConsistentGroups = []
        vbConsistentGroup = [False] * len(self.mvConsistentGroups)
        for cand in vpCandidateKFs:
            spCandidateGroup = set(self.connected(cand)) | {cand}
            bEnoughConsistent = False
            bConsistentForSomeGroup = False
            for iG, (sPreviousGroup, n) in enumerate(self.mvConsistentGroups):
                if spCandidateGroup & sPreviousGroup:
                    bConsistentForSomeGroup = True
                    nCurrentConsistency = n + 1
                    if not vbConsistentGroup[iG]:
                        vCurrentConsistentGroups.append((spCandidateGroup, nCurrentConsistency))
                        vbConsistentGroup[iG] = True
                    if nCurrentConsistency >= 3 and not bEnoughConsistent:
                        enough.append(cand)
                        bEnoughConsistent = True
            if not bConsistentForSomeGroup:
                vCurrentConsistentGroups.append((spCandidateGroup, 0))
        self.mvConsistentGroups = vCurrentConsistentGroups
        self.added.append(mnId)
        return bool(enough), enough
