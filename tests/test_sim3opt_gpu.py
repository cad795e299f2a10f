"""GPU Optimizer::OptimizeSim3 (orbo_*: both optimize() calls, the outlier removal between them and the
final count in one launch, Optimizer.cc:1405-1637) against the float64 numpy restatement of
tests/sim3opt_ref.py in its reference mode (g2o's central differences at 1e-9, edges summed in order).

Gates: the removal state on decided pairs (BAND = 2.8e-4 of th2, derived in sim3opt_ref.py from the
reference's own mode-to-mode deviation), n_inliers within the number of undecided pairs, s R, t and s
within RTOL = 1e-4 relative (the project's contract), LM iterations within +-1 per stage."""
import numpy as np
import pytest

import sim3opt_ref as ref
from orbslam2_amd import synth

pytestmark = pytest.mark.gpu

RTOL = ref.RTOL


@pytest.fixture(scope="module")
def opt(amd):
    o = amd.Sim3Optimizer()
    yield o
    o.close()


def _bytes(out):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("q", "t", "s", "state", "chi2")) + \
        repr((out["n_inliers"], tuple(out["iterations"]))).encode()


def check_against_reference(prob, out):
    r = ref.reference(prob)
    n = len(prob["X1c"])
    d1, d2 = ref.decided(prob)
    und = int((~d2).sum())
    Mg, sg = ref.result_matrix(out)
    Mr, sr = ref.result_matrix(r)
    dsR = np.abs(Mg[:, :3] - Mr[:, :3]).max() / np.abs(Mr[:, :3]).max()
    dt = np.abs(Mg[:, 3] - Mr[:, 3]).max() / max(np.abs(Mr[:, 3]).max(), 1e-300)
    ds = abs(sg - sr) / sr
    with np.errstate(all="ignore"):
        dchi = np.abs(out["chi2"] - r["chi2"]) / np.abs(r["chi2"])
    print(f"n={n} fix={int(prob['fix_scale'])}: iterations gpu {tuple(out['iterations'])} ref {r['iterations']}, n_inliers gpu "
          f"{out['n_inliers']} ref {r['n_inliers']}, undecided {int((~d1).sum())}/{und}, relative deviation sR {dsR:.3e} "
          f"t {dt:.3e} s {ds:.3e} (RTOL {RTOL:.0e}), chi2 {np.nanmax(dchi) if n else 0:.3e} (BAND {ref.BAND:.1e})")
    assert out["state"].shape == (n,) and set(np.unique(out["state"])) <= {0, 1, 2}
    assert d1.all(), "every pair is decided at stage 1 by construction"
    np.testing.assert_array_equal(out["state"] == 1, r["state"] == 1)
    np.testing.assert_array_equal(out["state"][d2], r["state"][d2])
    assert abs(out["n_inliers"] - r["n_inliers"]) <= und
    assert out["n_inliers"] == int((out["state"] == 0).sum()) or out["iterations"][1] == -1
    for a, b in zip(out["iterations"], r["iterations"]):
        assert (a > 0) == (b > 0) and abs(a - b) <= 1
    assert dsR <= RTOL and dt <= RTOL and ds <= RTOL
    if bool(prob["fix_scale"]) and float(prob["s"]) == 1.0:
        assert out["s"] == 1.0
    return r


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=[f"n{n}-fix{f}" for n, f in ref.CASES])
def test_matches_reference(opt, k):
    prob = ref.case_problem(k)
    r = check_against_reference(prob, opt.optimize(prob))
    assert r["iterations"][1] > 0
    if ref.CASES[k][0] == 12:
        assert r["n_inliers"] == 10 and (r["state"] == 1).sum() == 2     # exactly 10 survivors: stage 2 runs


@pytest.mark.parametrize("k", [0, 1])
def test_different_intrinsics(opt, k):
    prob = ref.k2_problem(k)
    assert not np.array_equal(prob["K1"], prob["K2"])
    check_against_reference(prob, opt.optimize(prob))


def test_clean_set_runs_five_more(opt):
    """No pair removed: nBad == 0, so the second optimize is optimize(5)."""
    prob = ref.clean_problem()
    out = opt.optimize(prob)
    check_against_reference(prob, out)
    assert not out["state"].any() and out["n_inliers"] == len(prob["X1c"])
    assert 0 < out["iterations"][1] <= 5


def test_return_zero_after_stage1(opt):
    """n = 11, two outliers: 9 survivors, `return 0` (Optimizer.cc:1605) with g2oS12 untouched but the
    stage-1 removals done."""
    prob = ref.return0_problem()
    r = ref.reference(prob)
    assert r["n_inliers"] == 0 and r["iterations"][1] == -1 and (r["state"] == 1).sum() == 2
    out = opt.optimize(prob)
    assert out["n_inliers"] == 0
    assert out["q"].tobytes() == np.asarray(prob["q"], np.float64).tobytes()
    assert out["t"].tobytes() == np.asarray(prob["t"], np.float64).tobytes()
    assert np.float64(out["s"]).tobytes() == np.float64(prob["s"]).tobytes()
    np.testing.assert_array_equal(out["state"], r["state"])
    assert out["iterations"][1] == -1 and abs(out["iterations"][0] - r["iterations"][0]) <= 1
    np.testing.assert_array_equal((out["chi2"] > float(prob["th2"])).any(1), out["state"] == 1)   # what the kernel compared


def test_fewer_than_ten_pairs(opt):
    """1 <= n < 10 still runs the first optimize and reports its removals, then returns 0."""
    prob = synth.optimize_sim3_problem(ref.SEED0 + 60, n=7, fix_scale=True, n_outliers=1)
    r = ref.optimize_sim3(prob)
    out = opt.optimize(prob)
    assert out["n_inliers"] == 0 and out["iterations"][0] > 0 and out["iterations"][1] == -1
    np.testing.assert_array_equal(out["state"], r["state"])
    assert (out["state"] == 1).sum() == 1
    assert out["q"].tobytes() == np.asarray(prob["q"], np.float64).tobytes()


def test_empty_problem(opt):
    prob = dict(ref.case_problem(1))
    for k in ("X1c", "X2c", "obs1", "obs2"):
        prob[k] = prob[k][:0]
    for k in ("inv_sigma2_1", "inv_sigma2_2"):
        prob[k] = prob[k][:0]
    out = opt.optimize(prob)
    assert out["n_inliers"] == 0 and tuple(out["iterations"]) == (-1, -1) and len(out["state"]) == 0
    assert out["q"].tobytes() == np.asarray(prob["q"], np.float64).tobytes()
    assert out["t"].tobytes() == np.asarray(prob["t"], np.float64).tobytes() and out["s"] == prob["s"]


def test_batched_and_repeatable(amd, opt):
    """All problems in 12 slots of one launch: byte-identical to the single calls, whatever the slot;
    a second run repeats the first bit for bit."""
    probs = ref.all_problems()
    assert len(probs) >= 8
    want = [_bytes(opt.optimize(p)) for p in probs]
    b = amd.Sim3Optimizer()
    got = b.optimize_batch(probs)
    assert [_bytes(g) for g in got] == want
    b.run_batch(len(probs))
    assert [_bytes(b.fetch(s, len(p["X1c"]))) for s, p in enumerate(probs)] == want
    rev = b.optimize_batch(probs[::-1])[::-1]                                   # other slots, other neighbours
    assert [_bytes(g) for g in rev] == want
    b.close()


def chain_optimize_problem(prob, m12, R12, t12, s12):
    """The edges Optimizer::OptimizeSim3 adds (Optimizer.cc:1469-1566) for vpMatches1 = m12 (SearchBySim3's
    output: the kf2 map point of each kf1 keypoint, or -1) -> (problem dict, vnIndexEdge)."""
    k1, k2 = prob["kf1"], prob["kf2"]
    first2 = {}
    for j, p in enumerate(prob["kf2_mp"]):
        if p >= 0 and int(p) not in first2:
            first2[int(p)] = j                                                   # GetIndexInKeyFrame
    bad = prob["map"]["flags"] & synth.MP_BAD
    rows = [(i, first2[int(m)], int(prob["kf1_mp"][i]), int(m)) for i, m in enumerate(m12)
            if m >= 0 and prob["kf1_mp"][i] >= 0 and not bad[prob["kf1_mp"][i]] and not bad[m] and int(m) in first2]
    i1, i2, mp1, mp2 = (np.array(c) for c in zip(*rows))

    def cam(k, mp):
        T = np.asarray(k["Tcw"], np.float32).reshape(-1)[:12].reshape(3, 4)
        Xw = prob["map"]["Xw"][mp].astype(np.float32)
        return ((Xw @ T[:, :3].T).astype(np.float32) + T[:, 3]).astype(np.float32)

    K = lambda k: np.array([k["fx"], k["fy"], k["cx"], k["cy"]], np.float32)
    pt = lambda k, idx: np.stack([k["keys_un"]["x"][idx], k["keys_un"]["y"][idx]], 1).astype(np.float32)
    op = {"X1c": cam(k1, mp1), "X2c": cam(k2, mp2), "obs1": pt(k1, i1), "obs2": pt(k2, i2),
          "inv_sigma2_1": np.asarray(k1["inv_level_sigma2"], np.float32)[k1["keys_un"]["octave"][i1]],
          "inv_sigma2_2": np.asarray(k2["inv_level_sigma2"], np.float32)[k2["keys_un"]["octave"][i2]],
          "K1": K(k1), "K2": K(k2), "q": ref.quat_from_R(np.asarray(R12, np.float64)),   # g2o::Sim3(R, t, s)
          "t": np.asarray(t12, np.float64), "s": float(s12), "th2": np.float32(10), "fix_scale": True}
    return op, i1


def test_chain_ransac_search_optimize(amd, opt):
    """LoopClosing::ComputeSim3's steps 2-4 chained: the Sim3Solver hit -> SearchBySim3(.., 7.5) ->
    OptimizeSim3 on those matches with th2 = 10 accepts the loop (nInliers >= 20), and SearchBySim3
    with the optimised Sim3 finds at least what it found with the RANSAC Sim3, minus 5 %."""
    import test_sim3solver_gpu as chain
    prob, sp = chain.chain_problem(chain.CHAIN_SEED)
    n = len(sp["X1c"])
    solver = amd.Sim3Solver()
    out = solver.evaluate(sp)
    solver.close()
    hit, no_more, nin, st = amd.Sim3Solver.iterate(out["n_inliers"], 300, N=n)
    assert hit >= 0
    t = amd.Tracker()
    est = dict(prob)
    est.update(R12=out["R12"][hit], t12=out["t12"][hit], s12=np.float32(out["s12"][hit]))
    nf_ransac, m12 = t.search_by_sim3(est, 7.5)
    op, idx = chain_optimize_problem(prob, m12, out["R12"][hit], out["t12"][hit], out["s12"][hit])
    res = opt.optimize(op)
    r = ref.optimize_sim3(op)
    print(f"chain: {len(idx)} pairs from {nf_ransac} SearchBySim3 matches, OptimizeSim3 n_inliers {res['n_inliers']} "
          f"(restatement {r['n_inliers']}), iterations {res['iterations']}")
    assert res["n_inliers"] >= 20
    d1, d2 = ref.decided(op)
    if d1.all():                                                                 # else the stage-2 problems may differ
        assert abs(res["n_inliers"] - r["n_inliers"]) <= int((~d2).sum())
    opt_est = dict(prob)
    opt_est.update(R12=ref.quat_to_R(res["q"]).astype(np.float32), t12=res["t"].astype(np.float32), s12=np.float32(res["s"]))
    nf_opt, _ = t.search_by_sim3(opt_est, 7.5)
    print(f"chain: SearchBySim3 finds {nf_opt} with the optimised Sim3 ({nf_ransac} with the RANSAC Sim3)")
    assert nf_opt >= nf_ransac - 0.05 * nf_ransac
