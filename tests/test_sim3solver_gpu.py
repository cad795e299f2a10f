"""GPU Sim3Solver (orbs_*: Sim3Solver::ComputeSim3 + CheckInliers for every RANSAC hypothesis in one
launch, Sim3Solver.cc:330-488) against the float64 numpy reference of tests/sim3_ref.py, inside the
band that module derives from its own float32-vs-float64 deviation (BAND = 2.2 % of a threshold,
T_TOL = 4.2e-3 on [s R | t]; well-conditioned = float64 eigengap >= 1e-3)."""
import numpy as np
import pytest

import sim3_ref as ref
from orbslam2_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(amd):
    s = amd.Sim3Solver()
    yield s
    s.close()


def _same(a: dict, b: dict):
    for k in ("n_inliers", "inlier_bits", "R12", "t12", "s12"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def check_against_reference(amd, prob, out, caps=True):
    """The per-hypothesis contract; returns the GPU inlier matrix [H, n]."""
    r = ref.reference(prob, "f64")
    n, H = len(prob["X1c"]), len(prob["triplets"])
    bits = out["inlier_bits"]
    assert bits.shape == (H, (n + 63) // 64)
    full = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not full[:, n:].any(), "bits >= n set"
    inl = full[:, :n]
    np.testing.assert_array_equal(out["n_inliers"], inl.sum(1))                  # count = popcount
    np.testing.assert_array_equal(inl, amd.Sim3Solver.unpack_bits(bits, n))
    wc = ref.well_conditioned(r)
    dec = ref.decided(prob, r)
    undecided = ~dec & wc[:, None]
    print(f"n={n} H={H}: undecided {undecided.sum()} of {dec.size}, ill-conditioned {(~wc).sum()}, "
          f"mask differences {(inl != r['inliers'])[wc].sum()} (decided: {((inl != r['inliers']) & dec).sum()})")
    assert not ((inl != r["inliers"]) & dec).any()
    dcount = np.abs(out["n_inliers"].astype(np.int64) - r["n_inliers"])
    assert (dcount[wc] <= undecided.sum(1)[wc]).all()
    sR = out["s12"][:, None, None].astype(np.float64) * out["R12"]
    dT = np.maximum(np.abs(sR - r["T12"][:, :, :3]).reshape(H, -1).max(1), np.abs(out["t12"] - r["T12"][:, :, 3]).max(1))
    print(f"   largest |d[sR|t]| over well-conditioned hypotheses {dT[wc].max() if wc.any() else 0:.3e} (T_TOL {ref.T_TOL:.1e})")
    assert (dT[wc] <= ref.T_TOL).all()
    if bool(prob["fix_scale"]):
        assert (out["s12"] == 1.0).all()
    if caps:
        assert undecided.sum() <= 0.01 * dec.size
        assert (~wc).sum() <= 0.02 * H
    return inl


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=[f"n{n}-h{h}-fix{f}" for n, h, f in ref.CASES])
def test_hypotheses_match_reference(amd, solver, k):
    prob = ref.case_problem(k)
    check_against_reference(amd, prob, solver.evaluate(prob))


@pytest.mark.parametrize("k", [4, 6])
def test_different_intrinsics(amd, solver, k):
    prob = ref.case_problem(k, True)
    assert not np.array_equal(prob["K1"], prob["K2"])
    check_against_reference(amd, prob, solver.evaluate(prob))


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=[f"n{n}-h{h}-fix{f}" for n, h, f in ref.CASES])
def test_iterate_scan(amd, solver, k):
    """The replayed iterate(5) sequence: the reference's iteration index, nInliers, bNoMore pattern and
    vbInliers on decided entries. SetRansacParameters(0.99, 20, n_hyp): the case's hypotheses are all
    the solver may use."""
    n, H, fix = ref.CASES[k]
    prob = ref.case_problem(k)
    r = ref.reference(prob, "f64")
    out = solver.evaluate(prob)
    cand, hit_r, nin_r, log_r = ref.round_robin([ref.Scan(n, r["n_inliers"], max_iterations=H)])
    st, log = None, []
    while True:
        hit, no_more, nin, st = amd.Sim3Solver.iterate(out["n_inliers"], 5, state=st, N=n, max_iterations=H)
        log.append((0, hit, no_more))
        if hit >= 0 or no_more:
            break
    assert log == log_r
    assert hit == hit_r and nin == nin_r
    if hit >= 0:
        inl = amd.Sim3Solver.unpack_bits(out["inlier_bits"], n)[hit]
        dec = ref.decided(prob, r)[hit]
        np.testing.assert_array_equal(inl[dec], r["inliers"][hit][dec])
        assert st["best"] == hit


def test_hostile_inputs(amd, solver):
    """Coincident and collinear triplets, z = 0, negative depth, K1 != K2: the coincident triplet gives
    0 inliers and NaN falls out through the comparison alone; every other hypothesis is unaffected
    (the contract holds for all of them); points at negative depth are inliers where the reference
    says so."""
    prob = ref.hostile_problem()
    r = ref.reference(prob, "f64")
    out = solver.evaluate(prob)
    inl = check_against_reference(amd, prob, out, caps=False)
    h = ref.HOSTILE_COINCIDENT
    assert out["n_inliers"][h] == 0 and not out["inlier_bits"][h].any()
    assert not inl[:, 20].any() and not inl[:, 21].any()                 # z = 0
    dec = ref.decided(prob, r)
    b = prob["behind"]
    np.testing.assert_array_equal(inl[:, b][dec[:, b]], r["inliers"][:, b][dec[:, b]])
    assert inl[:, b][dec[:, b]].any()                                     # some are inliers, as the reference says
    # the same problem without the planted triplets: the other hypotheses' outputs are bit-identical
    clean = dict(prob)
    t = prob["triplets"].copy()
    t[ref.HOSTILE_COINCIDENT] = t[0]
    t[ref.HOSTILE_COLLINEAR] = t[1]
    clean["triplets"] = t
    out2 = solver.evaluate(clean)
    keep = np.ones(len(t), bool)
    keep[[ref.HOSTILE_COINCIDENT, ref.HOSTILE_COLLINEAR]] = False
    for key in ("n_inliers", "inlier_bits", "R12", "t12", "s12"):
        assert out[key][keep].tobytes() == out2[key][keep].tobytes(), key


def test_batched(amd):
    """7 slots with different n, n_hyp and fix_scale: each fetch equals its own orbs_evaluate bit for
    bit; after a re-stage of slot 3 with a smaller problem nothing of the old one remains."""
    probs = [ref.case_problem(k) for k in range(1, 8)]
    single = amd.Sim3Solver()
    want = [single.evaluate(p) for p in probs]
    b = amd.Sim3Solver()
    b.reserve(len(probs), 1000, 300)
    for s, p in enumerate(probs):
        b.stage(s, p)
    b.run_batch(len(probs))
    for s, p in enumerate(probs):
        _same(b.fetch(s, len(p["X1c"]), len(p["triplets"])), want[s])
    small = ref.case_problem(1, True)
    assert len(small["X1c"]) < len(probs[3]["X1c"]) and len(small["triplets"]) < len(probs[3]["triplets"])
    b.stage(3, small)
    b.run_batch(len(probs))
    got = b.fetch(3, len(small["X1c"]), len(small["triplets"]))
    _same(got, single.evaluate(small))
    check_against_reference(amd, small, got, caps=False)
    for s, p in enumerate(probs):
        if s != 3:
            _same(b.fetch(s, len(p["X1c"]), len(p["triplets"])), want[s])
    single.close()
    b.close()


def chain_problem(seed):
    """Correspondences of LoopClosing::ComputeSim3 from synth.sim3_pair_problem: the map points both
    keyframes observe (what SearchByBoW would hand to the Sim3Solver constructor)."""
    prob = synth.sim3_pair_problem(seed, s12=1.0)
    k1, k2 = prob["kf1"], prob["kf2"]
    first2 = {}
    for j, p in enumerate(prob["kf2_mp"]):
        if p >= 0 and int(p) not in first2:
            first2[int(p)] = j
    rows = [(i, first2[int(p)], int(p)) for i, p in enumerate(prob["kf1_mp"])
            if p >= 0 and int(p) in first2 and not prob["map"]["flags"][p] & synth.MP_BAD]
    i1, i2, mp = (np.array(c) for c in zip(*rows))
    Xw = prob["map"]["Xw"][mp].astype(np.float32)

    def cam(k):
        T = np.asarray(k["Tcw"], np.float32).reshape(-1)[:12].reshape(3, 4)
        return ((Xw @ T[:, :3].T).astype(np.float32) + T[:, 3]).astype(np.float32)

    sigma2 = (np.asarray(k1["scale_factors"], np.float32) ** 2).astype(np.float32)
    thr = lambda o: np.floor(9.210 * sigma2[o].astype(np.float64)).astype(np.float32)
    n = len(rows)
    n_hyp = ref.ransac_iterations(n)
    rng = np.random.default_rng(seed + 7)
    trip = np.argsort(rng.random((n_hyp, n)), axis=1)[:, :3].astype(np.int32)
    K = lambda k: np.array([k["fx"], k["fy"], k["cx"], k["cy"]], np.float32)
    sp = {"X1c": cam(k1), "X2c": cam(k2), "max_err1": thr(k1["keys_un"]["octave"][i1]),
          "max_err2": thr(k2["keys_un"]["octave"][i2]), "K1": K(k1), "K2": K(k2), "fix_scale": True, "triplets": trip}
    return prob, sp


CHAIN_SEED = 80


def test_chain_into_search_by_sim3(amd, solver):
    """What the feature is for: the Sim3 of the RANSAC, fed to the existing SearchBySim3(.., 7.5), finds
    at least as many matches as the problem's own ground-truth R12 / t12, minus 5 %."""
    prob, sp = chain_problem(CHAIN_SEED)
    n = len(sp["X1c"])
    assert n > 100
    out = solver.evaluate(sp)
    hit, no_more, nin, st = amd.Sim3Solver.iterate(out["n_inliers"], 300, N=n)
    assert hit >= 0 and nin > 20
    t = amd.Tracker()
    nf_truth, _ = t.search_by_sim3(prob, 7.5)
    est = dict(prob)
    est.update(R12=out["R12"][hit], t12=out["t12"][hit], s12=np.float32(out["s12"][hit]))
    nf_est, _ = t.search_by_sim3(est, 7.5)
    print(f"chain: N={n}, hypothesis {hit} with {nin} inliers, SearchBySim3 finds {nf_est} (ground truth {nf_truth})")
    assert nf_truth > 20
    assert nf_est >= nf_truth - 0.05 * nf_truth
