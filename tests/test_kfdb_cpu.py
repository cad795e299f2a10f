"""KeyFrameDatabase without a GPU: the restatement tests/kfdb_ref.py agrees with the brute-force formulation
the GPU library uses, the word-count threshold is float arithmetic, the orbd_* C-ABI rejects bad arguments
before touching a device, the header / binding / library agree on the orbd_* set, and LoopClosing::DetectLoop's
consistency groups (C++ host layer over a table stand-in) equal a Python restatement."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kfdb_ref as ref
from orbslam2_amd import synth

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "orb-slam2-noted_amd" / "build" / "kfdb_test"


def _exe():
    if not EXE.exists():
        import __graft_entry__
        __graft_entry__.build()
    return str(EXE)


@pytest.mark.parametrize("seed,n_words,wpk", [(0, 64, (5, 30)), (1, 500, (10, 60)), (2, 5000, (0, 90))])
def test_inverted_file_walk_equals_brute_force(seed, n_words, wpk):
    """lKFsSharingWords (order and counts) by the reference's inverted-file walk == set intersections ordered by
    (first common word, add sequence), on random databases, again after erase and erase + re-add."""
    prob = synth.kfdb_problem(seed, n_kf=120, n_words_vocab=n_words, words_per_kf=wpk, n_places=4, n_queries=10)
    rng = np.random.default_rng(seed)
    db = ref.KeyFrameDatabase(n_words)
    for k in prob["keyframes"]:
        db.add(k["id"], k["words"], k["values"])

    def check(tag):
        nonempty = 0
        for q in prob["queries"]:
            conn = q.get("connected", ())
            walk, brute = db.sharing_words(q["words"], conn), db.brute_force(q["words"], conn)
            assert walk == brute, (tag, walk, brute)
            nonempty += bool(walk[0])
            # and the stateful restatement sees the same counts
            r = db.query(q)
            counts = dict(zip(*walk))
            assert all(counts[i] == w for i, w in zip(r["scored_ids"].tolist(), r["scored_words"].tolist()))
            if walk[0]:
                assert r["max_common_words"] == max(walk[1])
        assert nonempty >= 5, tag

    check("fresh")
    by_id = {k["id"]: k for k in prob["keyframes"]}
    gone = rng.permutation(120)[:40].tolist()
    for i in gone:
        db.erase(i)
    check("erased")
    for i in rng.permutation(gone)[:25].tolist():     # back in another order: they move to the end of every list
        db.add(i, by_id[i]["words"], by_id[i]["values"])
    check("re-added")


def test_min_common_words_is_float_arithmetic(tmp_path):
    """int minCommonWords = maxCommonWords * 0.8f for 1..2000: the restatement's np.float32 product, the C++
    statement itself, and exact integer arithmetic (0.8f = 13421773 / 2^24, product rounded to 24 bits) agree."""
    subprocess.run([_exe(), "mincw", "2000", str(tmp_path / "m.txt")], check=True, timeout=60)
    cpp = [int(x) for x in (tmp_path / "m.txt").read_text().split()]
    assert len(cpp) == 2000

    def exact(m):
        p = m * 13421773                      # scaled by 2^24, fewer than 48 bits
        drop = max(p.bit_length() - 24, 0)
        q, rem = p >> drop, p & ((1 << drop) - 1)
        half = 1 << (drop - 1) if drop else 0
        if drop and (rem > half or (rem == half and q & 1)):
            q += 1
        return (q << drop) >> 24
    for m in range(1, 2001):
        assert ref.min_common_words(m) == cpp[m - 1] == exact(m), m
    assert ref.min_common_words(10) == 8 and ref.min_common_words(5) == 4      # 0.8f > 0.8: 10 * 0.8f rounds to 8.0f


def test_score_restatement():
    """L1Scoring::score: identical vectors -> 1, disjoint -> -0.0 (the reference returns -score / 2.0 of +0.0),
    and the skip-ahead walk equals the sum over the intersection in ascending word order."""
    rng = np.random.default_rng(3)
    w = np.sort(rng.choice(1000, 200, replace=False))
    v = rng.uniform(0.1, 1, 200)
    v /= v.sum()
    assert abs(float(ref.score(list(w), list(v), list(w), list(v))) - 1) < 1e-6
    z = ref.score([1, 3], [0.5, 0.5], [2, 4], [0.5, 0.5])
    assert z == 0 and np.signbit(z)
    w2 = np.sort(rng.choice(1000, 300, replace=False))
    v2 = rng.uniform(0.1, 1, 300)
    v2 /= v2.sum()
    d1, d2 = dict(zip(w.tolist(), v.tolist())), dict(zip(w2.tolist(), v2.tolist()))
    s = 0.0
    for k in sorted(set(d1) & set(d2)):
        s += (abs(d1[k] - d2[k]) - abs(d1[k])) - abs(d2[k])
    assert ref.score(w.tolist(), v.tolist(), w2.tolist(), v2.tolist()).tobytes() == np.float32(-s / 2.0).tobytes()


def test_synth_problem_shape():
    p = synth.kfdb_problem(5, n_kf=50, n_words_vocab=300, words_per_kf=(0, 40), n_queries=6)
    assert len(p["keyframes"]) == 50 and len(p["queries"]) == 6
    for k in p["keyframes"]:
        w = k["words"]
        assert w.dtype == np.uint32 and (np.diff(w.astype(np.int64)) > 0).all() and (w < 300).all()
        assert len(k["covisibles"]) <= 10 and k["values"].dtype == np.float64
        assert len(w) == 0 or abs(k["values"].sum() - 1) < 1e-12
    assert {q["kind"] for q in p["queries"]} == {0, 1}
    assert any(57 in k["covisibles"] for k in p["keyframes"])        # an id that is never added


def test_orbd_argument_errors_without_gpu():
    """ORBX_EINVAL before any device is touched: NULL pointers, words not strictly ascending, a word >= n_words,
    a negative kf_id, erase of an unknown id, covisibles of an unknown id, n > 10 covisibles, a slot out of range, an
    unsupported scoring type, a BowVector longer than ORBD_MAX_WORDS, an unknown query kind. (A duplicate kf_id
    needs a stored keyframe: tests/test_kfdb_gpu.py::test_argument_errors_with_keyframes.)"""
    import orbslam2_amd as amd
    lib = amd.lib()
    E = amd.ORBX_EINVAL
    h = C.c_void_p()
    assert lib.orbd_create(100, amd.ORBD_L1_NORM, None) == E
    for scoring in (1, 2, 3, 4, 5, -1):                 # L2_NORM .. DOT_PRODUCT
        assert lib.orbd_create(100, scoring, C.byref(h)) == E
    assert lib.orbd_create(0, amd.ORBD_L1_NORM, C.byref(h)) == E
    assert lib.orbd_create(100, amd.ORBD_L1_NORM, C.byref(h)) == 0 and h.value
    try:
        w = np.array([3, 7, 20], np.uint32)
        v = np.array([0.5, 0.25, 0.25])
        ids = np.arange(11, dtype=np.int64)
        n = C.c_int32(-1)
        assert lib.orbd_size(h, C.byref(n)) == 0 and n.value == 0
        assert lib.orbd_size(None, C.byref(n)) == E and lib.orbd_size(h, None) == E
        # add
        assert lib.orbd_add(None, 1, amd._p(w), amd._p(v), 3) == E
        assert lib.orbd_add(h, 1, None, amd._p(v), 3) == E
        assert lib.orbd_add(h, 1, amd._p(w), None, 3) == E
        assert lib.orbd_add(h, -1, amd._p(w), amd._p(v), 3) == E
        assert lib.orbd_add(h, 1, amd._p(w), amd._p(v), -1) == E
        assert lib.orbd_add(h, 1, amd._p(np.array([3, 3, 20], np.uint32)), amd._p(v), 3) == E       # not strictly ascending
        assert lib.orbd_add(h, 1, amd._p(np.array([7, 3, 20], np.uint32)), amd._p(v), 3) == E
        assert lib.orbd_add(h, 1, amd._p(np.array([3, 7, 100], np.uint32)), amd._p(v), 3) == E      # >= n_words
        big_w, big_v = np.arange(amd.ORBD_MAX_WORDS + 1, dtype=np.uint32), np.ones(amd.ORBD_MAX_WORDS + 1)
        hb = C.c_void_p()
        assert lib.orbd_create(10000, 0, C.byref(hb)) == 0
        assert lib.orbd_add(hb, 1, amd._p(big_w), amd._p(big_v), len(big_w)) == E
        lib.orbd_destroy(hb)
        assert lib.orbd_add_from_vocab(h, 1, None, 0) == E and lib.orbd_add_from_vocab(None, 1, None, 0) == E
        # erase / covisibles / clear
        assert lib.orbd_erase(None, 1) == E
        assert lib.orbd_erase(h, 1) == E                                 # unknown id
        assert lib.orbd_set_covisibles(h, 1, amd._p(ids), 2) == E        # unknown id
        assert lib.orbd_set_covisibles(h, 1, amd._p(ids), 11) == E       # n > 10
        assert lib.orbd_set_covisibles(h, 1, None, 2) == E and lib.orbd_set_covisibles(None, 1, amd._p(ids), 2) == E
        assert lib.orbd_set_covisibles(h, 1, amd._p(ids), -1) == E
        assert lib.orbd_clear(None) == E and lib.orbd_clear(h) == 0
        # queries
        Q, keep = amd.orbd_query({"kind": amd.ORBD_RELOC, "words": w, "values": v})
        R, out = amd.KeyFrameDatabase._result(4)
        assert lib.orbd_detect(None, C.byref(Q), C.byref(R)) == E
        assert lib.orbd_detect(h, None, C.byref(R)) == E
        assert lib.orbd_detect(h, C.byref(Q), None) == E
        R2, _ = amd.KeyFrameDatabase._result(4)
        R2.candidates = None
        assert lib.orbd_detect(h, C.byref(Q), C.byref(R2)) == E

        def bad(**kw):
            q = {"kind": amd.ORBD_LOOP, "words": w, "values": v, "connected": [1, 2], "min_score": 0.1}
            q.update({k: x for k, x in kw.items() if not k.startswith("_")})
            Q2, k2 = amd.orbd_query(q)
            for f, x in kw.items():
                if f.startswith("_"):
                    setattr(Q2, f[1:], x)
            return lib.orbd_detect(h, C.byref(Q2), C.byref(R)), lib.orbd_stage(h, 0, C.byref(Q2))

        assert lib.orbd_reserve(None, 2) == E and lib.orbd_reserve(h, 0) == E
        assert lib.orbd_stage(h, 0, C.byref(Q)) == E                     # nothing reserved: no such slot
        assert lib.orbd_run_batch(h, 1, None) == E
        assert lib.orbd_reserve(h, 2) == 0                               # host bookkeeping only
        assert bad(_words=None) == (E, E) and bad(_values=None) == (E, E)
        assert bad(_connected=None) == (E, E) and bad(_n_connected=-1) == (E, E)
        assert bad(kind=2) == (E, E) and bad(kind=-1) == (E, E)
        assert bad(words=np.array([3, 3, 20], np.uint32)) == (E, E)
        assert bad(words=np.array([3, 7, 100], np.uint32)) == (E, E)
        assert bad(_n=-1) == (E, E) and bad(_n=amd.ORBD_MAX_WORDS + 1) == (E, E)
        assert lib.orbd_stage(None, 0, C.byref(Q)) == E and lib.orbd_stage(h, 0, None) == E
        assert lib.orbd_stage(h, 2, C.byref(Q)) == E and lib.orbd_stage(h, -1, C.byref(Q)) == E
        assert lib.orbd_stage_from_vocab(h, 0, C.byref(Q), None, 0) == E
        assert lib.orbd_stage_from_vocab(h, 2, C.byref(Q), None, 0) == E
        assert lib.orbd_run_batch(None, 1, None) == E and lib.orbd_run_batch(h, 3, None) == E and lib.orbd_run_batch(h, 0, None) == E
        assert lib.orbd_run_batch(h, 1, None) == amd.ORBX_ESTATE               # nothing staged
        assert lib.orbd_fetch(h, 2, C.byref(R)) == E and lib.orbd_fetch(h, -1, C.byref(R)) == E
        assert lib.orbd_fetch(h, 0, None) == E and lib.orbd_fetch(None, 0, C.byref(R)) == E
        assert lib.orbd_fetch(h, 0, C.byref(R)) == amd.ORBX_ESTATE       # nothing ran
        # scores
        sc, mn = np.zeros(4, np.float32), C.c_float(0)
        kid = np.array([1, 2], np.int64)
        assert lib.orbd_scores(None, amd._p(w), amd._p(v), 3, amd._p(kid), 2, amd._p(sc), C.byref(mn)) == E
        assert lib.orbd_scores(h, None, amd._p(v), 3, amd._p(kid), 2, amd._p(sc), C.byref(mn)) == E
        assert lib.orbd_scores(h, amd._p(w), amd._p(v), 3, None, 2, amd._p(sc), C.byref(mn)) == E
        assert lib.orbd_scores(h, amd._p(w), amd._p(v), 3, amd._p(kid), 2, None, C.byref(mn)) == E
        assert lib.orbd_scores(h, amd._p(w), amd._p(v), 3, amd._p(kid), 2, amd._p(sc), None) == E
        assert lib.orbd_scores(h, amd._p(w), amd._p(v), 3, amd._p(kid), -1, amd._p(sc), C.byref(mn)) == E
        assert lib.orbd_scores(h, amd._p(np.array([9, 7, 20], np.uint32)), amd._p(v), 3, amd._p(kid), 2, amd._p(sc),
                               C.byref(mn)) == E
        # unknown ids only: no device needed, minScore stays 1 and the scores read -1
        assert lib.orbd_scores(h, amd._p(w), amd._p(v), 3, amd._p(kid), 2, amd._p(sc), C.byref(mn)) == 0
        assert mn.value == 1.0 and sc[:2].tolist() == [-1, -1]
    finally:
        lib.orbd_destroy(h)
    lib.orbd_destroy(None)


def test_header_declares_orbd_abi():
    """The header declares exactly the orbd_* set, and every name is bound and exported."""
    import orbslam2_amd as amd
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "orbslam2_amd.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(orbd_[a-z_]+)\s*\(", text))
    assert names == {"orbd_create", "orbd_destroy", "orbd_add", "orbd_add_from_vocab", "orbd_erase", "orbd_clear",
                     "orbd_size", "orbd_set_covisibles", "orbd_detect", "orbd_reserve", "orbd_stage",
                     "orbd_stage_from_vocab", "orbd_run_batch", "orbd_fetch", "orbd_scores"}
    bound = {n for n, _, _ in amd.SIGNATURES}
    assert names <= bound and {n for n in bound if n.startswith("orbd_")} == names
    assert all(hasattr(amd.lib(), n) for n in names)
    for struct, cname in ((amd.OrbdQuery, "orbd_query"), (amd.OrbdResult, "orbd_result")):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", text).group(1)
        fields = re.findall(r"\*?\b([a-z_]+)\s*;", body)
        assert fields == [f for f, _ in struct._fields_], cname


# 12 keyframes: (mnId, candidates DetectLoopCandidates returns, mLastLoopKFid set before the call or -1)
SCRIPT = [(3, [100], -1),             # gate: mnId < 0 + 10, the candidates are never asked for
          (9, [100], -1),
          (10, [100], -1),            # a first group, consistency 0
          (11, [101], -1),            # 101's group shares 150 with 100's: 1
          (12, [102, 400], -1),       # 2, and an unrelated group at 0
          (13, [103, 200], -1),       # 3: the third consistent detection -> loop, candidate 103
          (14, [], -1),               # no candidates: the groups are reset
          (15, [103], -1),            # starts again at 0
          (16, [300, 301], -1),       # neither consistent with 103's group: both 0
          (17, [302, 303], -1),       # both consistent with both previous groups: each previous group counted once
          (18, [304], 9),             # CorrectLoop set mLastLoopKFid = 9: 18 < 19, gated
          (19, [304], -1)]            # the groups of keyframe 17 are still the previous ones: 2, once per previous group
CONNECTED = {100: [150, 151], 101: [150], 102: [101, 152], 103: [102], 200: [201], 400: [401],
             300: [310], 301: [310, 311], 302: [310], 303: [311, 300], 304: [302]}


def test_detect_loop_consistency_groups(tmp_path):
    """LoopClosing::DetectLoop (host C++) over a table stand-in for the database == the Python restatement, step by
    step: the +10 gate, the loop on the third consistent detection, the reset on an empty candidate list, one
    current group per previous group, the add of the keyframe on every path, minScore handed through."""
    min_scores = {i: np.float32(0.01 * (k + 1)) for k, (i, _, _) in enumerate(SCRIPT)}
    lines = [str(len(CONNECTED))]
    for i, c in CONNECTED.items():
        lines.append(f"{i} {len(c)} " + " ".join(map(str, c)))
    lines.append(str(len(SCRIPT)))
    for i, cands, last in SCRIPT:
        lines.append(f"{i} {float(min_scores[i]).hex()} {len(cands)} " + " ".join(map(str, cands)) + f" {last}")
    (tmp_path / "script.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_exe(), "stub", str(tmp_path / "script.txt"), str(tmp_path / "out.txt")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = []
    for line in (tmp_path / "out.txt").read_text().splitlines():       # one spelling for the hex floats
        t = line.split(" ")
        if "minScore" in t:
            k = t.index("minScore") + 1
            t[k] = float.fromhex(t[k]).hex()
        got.append(" ".join(t))

    cand = {i: c for i, c, _ in SCRIPT}
    asked = []

    def candidates(i):
        asked.append(i)
        return cand[i]
    py = ref.DetectLoopRef(candidates, lambda c: CONNECTED[c])
    want, loops = [], []
    for i, _, last in SCRIPT:
        if last >= 0:
            py.mLastLoopKFid = last
        n_asked = len(asked)
        loop, enough = py.DetectLoop(i)
        loops.append(loop)
        line = f"{i} {int(loop)} enough" + "".join(f" {e}" for e in enough) + " groups"
        for members, n in py.mvConsistentGroups:
            line += f" {n}:" + "".join(f"{m}," for m in sorted(members))
        if len(asked) > n_asked:
            line += f" minScore {float(min_scores[i]).hex()}"
        want.append(line + f" added {len(py.added)}")
    assert got == want
    assert loops == [False] * 5 + [True] + [False] * 6              # the loop on the third consistent detection
    assert asked == [10, 11, 12, 13, 14, 15, 16, 17, 19]            # gated keyframes never query
    assert want[6].startswith("14 0 enough 103 groups minScore")    # the reset on an empty candidate list (the member
                                                                    # list is cleared at :202 only, as in the reference)
    assert " 3:102,103," in want[5] and " 0:200,201," in want[5]
    assert want[9].count(":") == 2 and " 1:302,310," in want[9]      # one current group per previous group
    assert want[11].count(" 2:302,304,") == 2
    assert py.added == [i for i, _, _ in SCRIPT]
