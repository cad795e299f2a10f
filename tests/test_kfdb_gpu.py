"""KeyFrameDatabase on the GPU (orbd_*) against the CPU restatement tests/kfdb_ref.py: candidate ids and
order, lScoreAndMatch (ids, si, word counts), lAccScoreAndMatch (accScore, best keyframe) and the
orbd_scores floats and minimum, all by byte equality. No tolerance, no excluded case."""
import numpy as np
import pytest

import kfdb_ref as ref
from orbslam2_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ("candidates", "scored_ids", "scored_si", "scored_words", "acc_score", "acc_best")


def same(g, r, what=""):
    for k in KEYS:
        assert g[k].dtype == r[k].dtype and g[k].tobytes() == r[k].tobytes(), (what, k, g[k], r[k])
    assert (g["max_common_words"], g["min_common_words"]) == (r["max_common_words"], r["min_common_words"]), what


class Pair:
    """The GPU database and the restatement, fed the same calls."""

    def __init__(self, amd, n_words):
        self.g, self.r = amd.KeyFrameDatabase(n_words), ref.KeyFrameDatabase(n_words)

    def add(self, i, w, v, cov=None):
        self.g.add(i, w, v)
        self.r.add(i, w, v)
        if cov is not None:
            self.cov(i, cov)

    def cov(self, i, ids):
        self.g.set_covisibles(i, ids)
        self.r.set_covisibles(i, ids)

    def erase(self, i):
        self.g.erase(i)
        self.r.erase(i)

    def load(self, prob):
        for k in prob["keyframes"]:
            self.add(k["id"], k["words"], k["values"])
        for k in prob["keyframes"]:
            self.cov(k["id"], k["covisibles"])
        return self

    def query(self, q, what=""):
        g, r = self.g.detect(q), self.r.query(q)
        same(g, r, what)
        return r


def vec(rng, words, lo=0.1):
    w = np.array(sorted(set(int(x) for x in words)), np.uint32)
    v = rng.uniform(lo, 1.0, len(w))
    return w, v / v.sum() if len(v) else v


def reloc(w, v):
    return {"kind": ref.RELOC, "words": w, "values": v}


def loop(w, v, connected=(), min_score=0.0):
    return {"kind": ref.LOOP, "words": w, "values": v, "connected": list(connected), "min_score": min_score}


@pytest.mark.parametrize("n_kf", [1, 63, 64, 65, 257])
def test_keyframe_counts(amd, n_kf):
    prob = synth.kfdb_problem(n_kf, n_kf=n_kf, n_words_vocab=1000, words_per_kf=(20, 60), n_places=4, n_queries=6)
    p = Pair(amd, prob["n_words"]).load(prob)
    assert len(p.g) == n_kf
    hits = 0
    for k, q in enumerate(prob["queries"]):
        hits += len(p.query(q, f"q{k}")["candidates"])
    assert hits > 0


def test_bowvector_lengths(amd):
    """Lengths 0, 1, 63, 64, 65 and 700 in one database, as keyframes and as queries."""
    rng = np.random.default_rng(1)
    p = Pair(amd, 1000)
    lens = [0, 1, 63, 64, 65, 700, 64, 65, 700, 1]
    for i, n in enumerate(lens):
        p.add(i, *vec(rng, rng.choice(1000, n, replace=False)), cov=[(i + 1) % len(lens), (i + 5) % len(lens)])
    seen = 0
    for n in lens[:6]:
        w, v = vec(rng, rng.choice(1000, n, replace=False))
        seen += len(p.query(reloc(w, v), f"reloc {n}")["scored_ids"])
        seen += len(p.query(loop(w, v, [2], 0.0), f"loop {n}")["scored_ids"])
    assert seen >= 8
    assert len(p.query(reloc(*vec(rng, [])))["candidates"]) == 0


def test_small_vocabulary_ties(amd):
    """64 words: every keyframe shares words with every query and many counts tie."""
    prob = synth.kfdb_problem(3, n_kf=100, n_words_vocab=64, words_per_kf=(10, 40), n_places=3, n_queries=8)
    p = Pair(amd, 64).load(prob)
    tied = 0
    for k, q in enumerate(prob["queries"]):
        r = p.query(q, f"q{k}")
        tied += len(r["scored_words"]) - len(set(r["scored_words"].tolist()))
    assert tied > 0


def test_large_vocabulary(amd):
    """10^6 words, ids up to n_words - 1."""
    n = 1_000_000
    rng = np.random.default_rng(4)
    p = Pair(amd, n)
    base = rng.choice(n - 1, 300, replace=False)
    for i in range(20):
        words = list(rng.choice(base, 150, replace=False)) + list(rng.integers(0, n, 50)) + ([n - 1] if i % 2 else [])
        p.add(i, *vec(rng, words), cov=[(i + 1) % 20, (i + 2) % 20])
    w, v = vec(rng, list(rng.choice(base, 200, replace=False)) + [n - 1])
    r = p.query(reloc(w, v))
    assert len(r["candidates"]) > 0 and r["max_common_words"] > 50
    w, v = vec(rng, [n - 1])   # only the last word: its keyframes, in add order
    r = p.query(reloc(w, v))
    assert r["scored_ids"].tolist() == list(range(1, 20, 2))
    p.query(loop(w, v, [1, 3], 0.0))


def test_duplicate_bowvectors_strict_ties(amd):
    """Equal BowVectors give equal scores: a neighbour with an equal score does not replace the group's
    best (strict >), and equal accScores do not raise bestAccScore."""
    rng = np.random.default_rng(5)
    w, v = vec(rng, range(0, 40))
    p = Pair(amd, 500)
    for i in range(6):
        p.add(i, w, v, cov=[(i + 1) % 6, (i + 2) % 6])
    p.add(6, *vec(rng, range(20, 70)), cov=[0])
    qw, qv = vec(rng, range(5, 45))
    for q in (reloc(qw, qv), loop(qw, qv, [], 0.0)):
        r = p.query(q)
        six = r["scored_si"][np.isin(r["scored_ids"], range(6))]
        assert len(six) == 6 and len(set(six.tobytes()[4 * k: 4 * k + 4] for k in range(6))) == 1
        assert (r["acc_best"][:6] == r["scored_ids"][:6]).all()      # ties keep the group's own keyframe
        assert r["candidates"].tolist()[:6] == list(range(6))


def test_min_score_equal_to_a_score(amd):
    """minScore set to an actual si: that keyframe stays (si >= minScore)."""
    prob = synth.kfdb_problem(6, n_kf=80, n_words_vocab=400, words_per_kf=(30, 50), n_places=2, n_queries=2)
    p = Pair(amd, 400).load(prob)
    q = prob["queries"][1]
    r0 = p.query(dict(q, min_score=0.0, connected=[]))
    si = np.sort(r0["scored_si"])
    assert len(si) >= 4 and si[0] < si[-1]
    ms = si[len(si) // 2]
    r = p.query(dict(q, min_score=float(ms), connected=[]))
    assert ms.tobytes() in [s.tobytes() for s in r["scored_si"]]
    assert 0 < len(r["scored_si"]) < len(si) and (r["scored_si"] >= ms).all()


def test_word_count_threshold_is_strict(amd):
    """maxCommonWords 10 -> minCommonWords (int)(10 * 0.8f) = 8: 8 shared words fail, 9 pass."""
    rng = np.random.default_rng(7)
    p = Pair(amd, 200)
    p.add(0, *vec(rng, range(0, 10)))
    p.add(1, *vec(rng, list(range(0, 8)) + [50, 51]))
    p.add(2, *vec(rng, list(range(0, 9)) + [60]))
    for q in (reloc(*vec(rng, range(0, 10))), loop(*vec(rng, range(0, 10)))):
        r = p.query(q)
        assert (r["max_common_words"], r["min_common_words"]) == (10, 8)
        assert r["scored_ids"].tolist() == [0, 2] and r["scored_words"].tolist() == [10, 9]


def test_early_exits(amd):
    rng = np.random.default_rng(8)
    p = Pair(amd, 300)
    assert len(p.query(reloc(*vec(rng, range(10))), "empty database")["candidates"]) == 0
    for i in range(5):
        p.add(i, *vec(rng, range(10 * i, 10 * i + 15)))
    for q in (reloc(*vec(rng, range(200, 230))), loop(*vec(rng, range(200, 230)))):
        r = p.query(q, "no shared word")
        assert r["max_common_words"] == 0 and len(r["scored_ids"]) == 0 and len(r["candidates"]) == 0
    r = p.query(loop(*vec(rng, range(0, 30)), [], 2.0), "nothing above minScore")
    assert r["max_common_words"] > 0 and len(r["scored_ids"]) == 0 and len(r["candidates"]) == 0
    r = p.query(loop(*vec(rng, range(0, 30)), range(5), 0.0), "every keyframe connected")
    assert r["max_common_words"] == 0 and len(r["candidates"]) == 0


def test_connected_set_excludes_top_scorer(amd):
    prob = synth.kfdb_problem(9, n_kf=90, n_words_vocab=600, words_per_kf=(30, 60), n_places=3, n_queries=2)
    p = Pair(amd, 600).load(prob)
    q = dict(prob["queries"][1], connected=[], min_score=0.0)
    r0 = p.query(q)
    top = int(r0["scored_ids"][np.argmax(r0["scored_si"])])
    r = p.query(dict(q, connected=[top]))
    assert top not in r["scored_ids"] and top not in r["acc_best"] and top not in r["candidates"]
    assert len(r["candidates"]) > 0


def _groups(amd):
    """A (0) and C (2) score low, their neighbour B (1) scores high: both groups' best is B."""
    rng = np.random.default_rng(10)
    p = Pair(amd, 400)
    q = vec(rng, range(0, 40))
    p.add(0, *vec(rng, list(range(0, 36)) + list(range(100, 140))), cov=[1])
    p.add(1, q[0], q[1] * 1.0, cov=[0])
    p.add(2, *vec(rng, list(range(2, 38)) + list(range(200, 240))), cov=[7, 1, 99])   # 7, 99: never added
    p.add(3, *vec(rng, range(300, 330)), cov=[0, 1, 2])
    return p, q


def test_neighbour_replaces_best_and_dedupe(amd):
    p, (qw, qv) = _groups(amd)
    for q in (reloc(qw, qv), loop(qw, qv, [], 0.0)):
        r = p.query(q)
        assert r["scored_ids"].tolist() == [0, 1, 2]
        assert r["acc_best"].tolist() == [1, 1, 1]            # the neighbour replaced the best of groups 0 and 2
        assert r["candidates"].tolist() == [1]                # one entry for three groups
    p.erase(1)                                                # an erased neighbour is skipped
    for q in (reloc(qw, qv), loop(qw, qv, [], 0.0)):
        r = p.query(q)
        assert r["acc_best"].tolist() == [0, 2] and r["acc_score"].tobytes() == r["scored_si"].tobytes()


def test_erase_and_readd_changes_order(amd):
    rng = np.random.default_rng(11)
    p = Pair(amd, 300)
    vs = [vec(rng, list(range(0, 20)) + [100 + i]) for i in range(5)]
    for i, (w, v) in enumerate(vs):
        p.add(i, w, v)
    q = reloc(*vec(rng, range(0, 20)))
    assert p.query(q)["scored_ids"].tolist() == [0, 1, 2, 3, 4]
    p.erase(1)
    p.add(1, *vs[1])
    assert p.query(q)["scored_ids"].tolist() == [0, 2, 3, 4, 1]
    p.erase(0)
    p.erase(3)
    p.add(3, *vs[3])
    p.add(0, *vs[0])
    assert p.query(q)["scored_ids"].tolist() == [2, 4, 1, 3, 0]
    p.g.clear()
    p.r.clear()
    assert len(p.g) == 0 and len(p.query(q)["scored_ids"]) == 0
    p.add(4, *vs[4])
    p.add(2, *vs[2])
    assert p.query(q)["scored_ids"].tolist() == [4, 2]


def test_growth_keeps_results(amd):
    """The slot table grows past 64 keyframes and the word pool past 65536 words (reallocate and copy):
    queries give the same results before and after, the mRelocScore state included."""
    rng = np.random.default_rng(12)
    p = Pair(amd, 5000)
    for i in range(60):
        p.add(i, *vec(rng, rng.choice(1000, 700, replace=False)), cov=[(i + 1) % 60, (i + 7) % 60])
    qa = reloc(*vec(rng, rng.choice(1000, 600, replace=False)))
    qb = reloc(*vec(rng, list(rng.choice(1000, 40, replace=False)) + list(range(2000, 2400))))
    p.add(1000, *vec(rng, range(2000, 2400)), cov=[0, 1, 2, 3])
    before = p.query(qa)
    stale = p.query(qb)                     # keyframe 1000's neighbours fail the threshold: stale scores from qa
    assert stale["scored_ids"].tolist() == [1000] and stale["acc_score"][0] > stale["scored_si"][0]
    p.query(qa)
    for i in range(60, 110):                # 111 keyframes, 77 400 words: both reallocations
        p.add(i, *vec(rng, 3000 + rng.choice(1000, 700, replace=False)))
    same(p.g.detect(qb), stale, "stale state after growth")
    p.r.query(qb)
    same(p.g.detect(qa), before, "after growth")
    p.r.query(qa)
    p.query(reloc(*vec(rng, 3000 + rng.choice(1000, 300, replace=False))))


def _chain(amd):
    """K (0) passes in q1; in q2 it shares one word and fails the threshold but is M's (1) neighbour;
    in q3 it passes again."""
    rng = np.random.default_rng(13)
    p = Pair(amd, 1000)
    p.add(0, *vec(rng, range(0, 10)), cov=[1])
    p.add(1, *vec(rng, range(100, 120)), cov=[0])
    qs = [reloc(*vec(rng, range(0, 10))), reloc(*vec(rng, list(range(100, 120)) + [3])), reloc(*vec(rng, range(0, 12)))]
    return p, qs


def test_reloc_chain_uses_stale_score(amd):
    p, qs = _chain(amd)
    r1, r2, r3 = (p.query(q, f"q{k}") for k, q in enumerate(qs))
    s1 = r1["scored_si"][0]
    assert r1["scored_ids"].tolist() == [0] and s1 > 0
    assert r2["scored_ids"].tolist() == [1] and r2["min_common_words"] == 16
    assert r2["acc_score"][0] == np.float32(r2["scored_si"][0] + s1)       # q1's score of K, not a fresh one
    assert r3["scored_ids"].tolist() == [0] and r3["scored_si"][0] != s1
    p.erase(0)                                                             # erase + add resets the state to 0.0f
    p.add(0, *vec(np.random.default_rng(14), range(0, 10)), cov=[1])
    r = p.query(qs[1])
    assert r["acc_score"][0] == r["scored_si"][0]


def test_reloc_chain_as_batch(amd):
    p, qs = _chain(amd)
    single = [p.query(q) for q in qs]
    p2, _ = _chain(amd)
    p2.g.reserve(3)
    for k, q in enumerate(qs):
        p2.g.stage(k, q)
    p2.g.run_batch(3)
    for k in range(3):
        same(p2.g.fetch(k), single[k], f"slot {k}")


def test_batch_of_17_mixed(amd):
    prob = synth.kfdb_problem(15, n_kf=150, n_words_vocab=800, words_per_kf=(30, 80), n_places=5, n_queries=17)
    a, b = Pair(amd, 800).load(prob), Pair(amd, 800).load(prob)
    assert {q["kind"] for q in prob["queries"]} == {ref.LOOP, ref.RELOC}
    single = [a.query(q, f"q{k}") for k, q in enumerate(prob["queries"])]
    b.g.reserve(17)
    for k, q in enumerate(prob["queries"]):
        b.g.stage(k, q)
    b.g.run_batch(17)
    for k in range(17):
        same(b.g.fetch(k), single[k], f"slot {k}")
    b.g.run_batch(5)                        # a second run continues from the state the first left, as 5 more calls do
    for k in range(5):
        same(b.g.fetch(k), a.query(prob["queries"][k]), f"rerun slot {k}")
    assert sum(len(s["candidates"]) for s in single) > 0


def test_scores(amd):
    prob = synth.kfdb_problem(16, n_kf=70, n_words_vocab=500, words_per_kf=(0, 90), n_places=3, n_queries=3)
    p = Pair(amd, 500).load(prob)
    for q in prob["queries"]:
        ids = [5, 0, 69, 500, 33, 5]        # 500 is not in the database; 5 twice
        g, gm = p.g.scores(q["words"], q["values"], ids)
        r, rm = p.r.scores(q["words"], q["values"], ids)
        assert g.tobytes() == r.tobytes() and np.float32(gm).tobytes() == np.float32(rm).tobytes()
        assert g[3] == -1 and rm < 1
    g, gm = p.g.scores(prob["queries"][0]["words"], prob["queries"][0]["values"], [])
    assert len(g) == 0 and gm == 1


def test_from_vocab_equals_host_staged(amd):
    """orbd_add_from_vocab / orbd_stage_from_vocab read the BowVectors orbv_transform_batch_device left in
    HBM; the results equal those of the same vectors fetched and passed through host memory."""
    import torch
    voc = synth.vocabulary(21, 6, 3)
    V = amd.Vocabulary(voc)
    nw = V.info()["n_words"]
    cap, F = 512, 12
    buf = np.zeros((F, cap, 32), np.uint8)
    cnt = np.zeros(F, np.int32)
    for f in range(F):
        d = synth.bow_features(voc, 200 + f, 120 + 30 * f)
        buf[f, : len(d)] = d
        cnt[f] = len(d)
    tb, tc = torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda()
    torch.cuda.synchronize()
    V.transform_batch_device(tb.data_ptr(), tc.data_ptr(), F, cap, cap * 32)
    bows = [V.batch_fetch(f, cap) for f in range(F)]
    assert all(len(b["words"]) > 20 for b in bows)
    dev, host = amd.KeyFrameDatabase(nw), Pair(amd, nw)
    for f in range(F - 3):
        dev.add_from_vocab(f, V, f)
        host.add(f, bows[f]["words"], bows[f]["values"])
    for f in range(F - 3):
        cov = [(f + 1) % (F - 3), (f + 4) % (F - 3)]
        dev.set_covisibles(f, cov)
        host.cov(f, cov)
    assert len(dev) == F - 3
    kinds = [reloc, lambda w, v: loop(w, v, [2], 0.0), reloc]
    dev.reserve(3)
    host.g.reserve(3)
    want = []
    for s in range(3):
        b = bows[F - 3 + s]
        q = kinds[s](b["words"], b["values"])
        dev.stage_from_vocab(s, dict(q, words=[], values=[]), V, F - 3 + s)
        host.g.stage(s, q)
        want.append(host.r.query(q))
        assert len(want[-1]["scored_ids"]) > 0
    dev.run_batch(3)
    host.g.run_batch(3)
    for s in range(3):
        same(host.g.fetch(s), want[s], f"host-staged slot {s}")
        same(dev.fetch(s), want[s], f"device-staged slot {s}")


def test_two_runs_identical(amd):
    prob = synth.kfdb_problem(18, n_kf=200, n_words_vocab=2000, words_per_kf=(50, 120), n_places=6, n_queries=6)
    out = []
    for _ in range(2):
        db = amd.KeyFrameDatabase(2000)
        for k in prob["keyframes"]:
            db.add(k["id"], k["words"], k["values"])
            db.set_covisibles(k["id"], [c for c in k["covisibles"]])
        res = [db.detect(q) for q in prob["queries"]]
        out.append(b"".join(r[k].tobytes() for r in res for k in KEYS))
    assert out[0] == out[1] and len(out[0]) > 100


def test_argument_errors_with_keyframes(amd):
    """The ORBX_EINVAL causes that need a stored keyframe: a duplicate kf_id, erase twice, covisibles of an erased
    id; and ORBX_ECAP with the counts filled in when the result arrays are too short."""
    import ctypes as C
    lib = amd.lib()
    rng = np.random.default_rng(20)
    db = amd.KeyFrameDatabase(100)
    w, v = vec(rng, range(0, 20))
    for i in range(3):
        db.add(i, w, v)
    assert lib.orbd_add(db._h, 1, amd._p(w), amd._p(v), len(w)) == amd.ORBX_EINVAL
    assert len(db) == 3
    db.erase(1)
    assert lib.orbd_erase(db._h, 1) == amd.ORBX_EINVAL
    assert lib.orbd_set_covisibles(db._h, 1, amd._p(np.array([0], np.int64)), 1) == amd.ORBX_EINVAL
    db.add(1, w, v)
    Q, keep = amd.orbd_query(reloc(w, v))
    R, out = amd.KeyFrameDatabase._result(2)
    assert lib.orbd_detect(db._h, C.byref(Q), C.byref(R)) == amd.ORBX_ECAP
    assert (R.n_scored, R.n_candidates) == (3, 3)
    assert db.detect(reloc(w, v))["candidates"].tolist() == [0, 2, 1]
