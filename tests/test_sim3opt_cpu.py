"""CPU checks of the Optimizer::OptimizeSim3 restatement (tests/sim3opt_ref.py), of the conditions its
cases must meet so that the GPU comparison is well posed, of synth.optimize_sim3_problem and of the
orbo_* argument checks, which return before the device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import sim3opt_ref as ref
from orbslam2_amd import synth


def test_reference_modes_agree():
    """The four modes (Jacobian step 1e-9 / 1e-6, edge order forward / reversed) give the same masks,
    counts and iteration counts on every problem, and their chi2 / Sim3 deviations stay inside the
    figures BAND and T_DEV are derived from."""
    near = anyd = tdev = 0.0
    for p in ref.all_problems():
        d = ref.mode_deviation(p)
        print(f"n={len(p['X1c'])} fix={int(p['fix_scale'])}: chi2 deviation {d['any_dev']:.2e} (within 4x of th2 {d['near_dev']:.2e}), "
              f"T deviation {d['t_dev']:.2e}, nearest chi2 to th2 {d['nearest']:.2e}, identical {d['identical']}")
        assert d["identical"]
        near, anyd, tdev = max(near, d["near_dev"]), max(anyd, d["any_dev"]), max(tdev, d["t_dev"])
    print(f"largest chi2 deviation {anyd:.2e} -> BAND {ref.BAND:.1e}; T deviation {tdev:.2e} (T_DEV {ref.T_DEV:.1e})")
    assert anyd <= ref.MEASURED_CHI2_DEV and ref.BAND == 4 * ref.MEASURED_CHI2_DEV
    assert tdev <= ref.T_DEV < ref.RTOL / 100


def test_case_conditions():
    """Every pair decided at stage 1 (a flipped stage-1 removal changes the stage-2 problem), at most
    1 % undecided at the final check, all projections finite, and the paths the cases are there for."""
    sizes = set()
    for p in ref.all_problems():
        r = ref.reference(p)
        n = len(p["X1c"])
        sizes.add(n)
        d1, d2 = ref.decided(p)
        assert d1.all()
        assert (~d2).sum() <= 0.01 * n
        assert all(ref.reference(p, m)["finite"] for m in ref.MODES)
        assert np.isfinite(r["chi2"]).all() and np.isfinite(r["chi2_stage1"]).all()
        np.testing.assert_array_equal(r["state"] > 0, p["outlier"])          # the planted outliers, nothing else
    assert {12, 70, 257, 300} <= sizes
    assert sum(not np.array_equal(p["K1"], p["K2"]) for p in ref.all_problems()) == 2
    for k, (n, fix) in enumerate(ref.CASES):
        p = ref.case_problem(k)
        assert len(p["X1c"]) == n and bool(p["fix_scale"]) == bool(fix) and float(p["th2"]) == ref.TH2
        if n == 12:
            r = ref.reference(p)
            assert (r["state"] == 1).sum() == 2 and r["n_inliers"] == 10 and r["iterations"][1] > 0
    r = ref.reference(ref.return0_problem())
    assert r["n_inliers"] == 0 and (r["state"] == 1).sum() == 2 and r["iterations"] == (r["iterations"][0], -1)
    p = ref.return0_problem()
    assert r["q"].tobytes() == np.asarray(p["q"], np.float64).tobytes() and r["s"] == p["s"]
    r = ref.reference(ref.clean_problem())
    assert not r["state"].any() and 0 < r["iterations"][1] <= 5


def test_reference_recovers_ground_truth():
    """The kept pairs end at the noise level: observations carry N(0, 0.6 px * scale) per axis and the
    information is 1 / scale^2, so a chi2 has mean 2 * 0.36 = 0.72 at the generating Sim3 (the mean over
    >= 20 edges stays below 1.5, five standard deviations up). With a fixed scale the Sim3 itself ends
    nearer the generating one than it started, and s stays exactly 1.0. A free scale is only weakly
    observable (|t| << depth), so there the reprojection is the yardstick, not s."""
    for p in ref.all_problems():
        r = ref.reference(p)
        if r["iterations"][1] < 0:
            continue
        kept = r["state"] == 0
        g = ref._Graph(p, "g2o", "forward")
        start_chi2 = g.chi2(g.errors((np.asarray(p["q"], np.float64), np.asarray(p["t"], np.float64), float(p["s"]))))
        print(f"n={len(p['X1c'])} fix={int(p['fix_scale'])}: mean chi2 of the kept pairs {start_chi2[kept].mean():.2f} -> "
              f"{r['chi2'][kept].mean():.2f}")
        assert r["chi2"][kept].mean() < 1.5 < start_chi2[kept].mean()
        if p["fix_scale"]:
            truth = np.concatenate([p["s12"] * p["R12"], p["t12"][:, None]], 1)
            start = ref.sim3_matrix((p["q"], p["t"], p["s"]))
            end, s = ref.result_matrix(r)
            assert np.abs(end - truth).max() < 0.5 * np.abs(start - truth).max()
            assert s == 1.0


def _exp_series(u, terms=30):
    """exp of the 4x4 generator [[sigma I + Omega, upsilon], [0, 0]] by its power series ->
    (s R, t): the closed form's yardstick."""
    w, ups, sigma = np.asarray(u[:3], np.float64), np.asarray(u[3:6], np.float64), float(u[6])
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + sigma * np.eye(3)
    G[:3, 3] = ups
    E, term = np.eye(4), np.eye(4)
    for k in range(1, terms):
        term = term @ G / k
        E = E + term
    return E[:3, :3], E[:3, 3]


@pytest.mark.parametrize("u, branch", [
    ([1e-9, 0, 0, 0.3, -0.2, 0.5, 0.0], 0),             # |sigma| < eps, theta < eps: the numeric Jacobian's branch
    ([2e-6, -3e-6, 1e-6, 0.3, -0.2, 0.5, 4e-6], 0),
    ([0.02, -0.015, 0.01, 0.3, -0.2, 0.5, 0.0], 1),     # |sigma| < eps, theta >= eps
    ([0.4, 0.2, -0.3, 1.0, 2.0, -0.5, 3e-6], 1),
    ([1e-7, 2e-7, 0, 0.3, -0.2, 0.5, 0.03], 2),         # |sigma| >= eps, theta < eps
    ([0.02, -0.015, 0.01, 0.3, -0.2, 0.5, -0.04], 3),   # the general branch: an accepted LM step with a free scale
    ([0.7, -0.4, 0.9, -1.0, 0.5, 2.0, 0.25], 3),
])
def test_sim3_exponential_branches(u, branch):
    assert ref.exp_branch(u) == branch
    q, t, s = ref.sim3_exp(np.array(u, np.float64))
    sR, ts = _exp_series(u)
    theta = math.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
    # the small-angle branches keep R = I + Omega + Omega^2 (second order wrong by theta^2 / 2) and
    # A = 1/2, B = 1/6 constants: the closed form is only accurate to the branch limit eps = 1e-5
    tol = 1e-12 if branch == 3 else (1e-12 if branch == 1 and abs(u[6]) == 0 else 2e-5 * max(1.0, np.abs(ts).max()))
    np.testing.assert_allclose(s * ref.quat_to_R(q), sR, atol=max(tol, theta ** 2), rtol=0)
    np.testing.assert_allclose(t, ts, atol=tol, rtol=0)
    if branch in (0, 2):
        assert abs(np.linalg.norm(q) - 1) <= theta ** 2 + 1e-15   # Quaterniond(R) of a non-rotation, not normalised
        w = np.array(u[:3])
        O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + O + O @ O
        assert np.array_equal(q, ref.quat_from_R(R))


def test_sim3_group_operations():
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        S = (q, rng.normal(0, 2, 3), float(rng.uniform(0.5, 2.0)))
        I = ref.sim3_mul(S, ref.sim3_inverse(S))
        np.testing.assert_allclose(I[0] * np.sign(I[0][3]), [0, 0, 0, 1], atol=1e-15)
        np.testing.assert_allclose(I[1], 0, atol=1e-14)
        assert abs(I[2] - 1) < 1e-15
        X = rng.normal(0, 5, (4, 3))
        np.testing.assert_allclose(ref.sim3_map(ref.sim3_inverse(S), ref.sim3_map(S, X)), X, atol=1e-13)
        qt = rng.normal(size=4)
        T = (qt / np.linalg.norm(qt), rng.normal(0, 2, 3), 1.3)
        np.testing.assert_allclose(ref.sim3_map(ref.sim3_mul(S, T), X), ref.sim3_map(S, ref.sim3_map(T, X)), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref.sim3_matrix(S)[:, :3], S[2] * ref.quat_to_R(q), atol=0)
        back = ref.quat_from_R(ref.quat_to_R(q))                   # q or -q: the pivot branch picks the sign
        np.testing.assert_allclose(back * np.sign(back @ q), q, atol=1e-14)
    # Sim3(0) * S reproduces S bit for bit: the scale column of a fixed-scale Jacobian is exactly zero
    Z = ref.oplus(S, np.array([0, 0, 0, 0, 0, 0, 1e-9]), True)
    assert Z[0].tobytes() == S[0].tobytes() and Z[1].tobytes() == S[1].tobytes() and Z[2] == S[2]


def test_ldlt_restatement():
    rng = np.random.default_rng(5)
    for _ in range(10):
        M = rng.normal(size=(7, 9))
        H = M @ M.T + 1e-3 * np.eye(7)
        b = rng.normal(size=7)
        np.testing.assert_allclose(ref.ldlt_solve(H, b), np.linalg.solve(H, b), rtol=1e-9)
    assert ref.ldlt_solve(-np.eye(7), np.ones(7)) is None                   # !isPositive()
    H = np.diag([3.0, 2.0, 1.0, 4.0, 5.0, 6.0, 1e-5])                       # fixed scale: H[6][6] = lambda alone
    np.testing.assert_array_equal(ref.ldlt_solve(H, np.array([1.0, 1, 1, 1, 1, 1, 0]))[6], 0.0)


def test_synth_problem_deterministic():
    a = synth.optimize_sim3_problem(11, n=50, fix_scale=False, outlier_frac=0.2, k2_differs=True)
    b = synth.optimize_sim3_problem(11, n=50, fix_scale=False, outlier_frac=0.2, k2_differs=True)
    for k, v in a.items():
        assert np.array_equal(np.asarray(v), np.asarray(b[k])), k
    c = synth.optimize_sim3_problem(12, n=50, fix_scale=False, outlier_frac=0.2, k2_differs=True)
    assert not np.array_equal(a["X1c"], c["X1c"])
    for k in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "K1", "K2"):
        assert a[k].dtype == np.float32, k
    assert a["X1c"].shape == (50, 3) and a["obs2"].shape == (50, 2) and a["outlier"].sum() == 10
    assert (a["X2c"][:, 2] >= 5).all() and (a["X2c"][:, 2] <= 30).all()
    assert not np.array_equal(a["K1"], a["K2"]) and abs(np.linalg.norm(a["q"]) - 1) < 1e-12
    assert 0.7 < a["s"] < 1.4 and a["s"] != a["s12"]
    f = synth.optimize_sim3_problem(11, n=50, fix_scale=True)
    assert f["s"] == 1.0 and f["s12"] == 1.0
    d = np.linalg.norm(a["obs2"].astype(np.float64) - (a["K2"][:2] * a["X2c"][:, :2] / a["X2c"][:, 2:] + a["K2"][2:]), axis=1)
    assert (d[a["outlier"]] >= 6).all() and (d[~a["outlier"]] < 8).all()


def test_orbo_argument_errors_without_gpu():
    """orbo_* return ORBX_EINVAL / ORBX_ECAP before touching the device: NULL pointers, n < 0, a bad slot,
    non-finite q / t / s, s <= 0, n > cap_pairs. orbo_create and orbo_reserve need no device."""
    import orbslam2_amd as amd
    lib = amd.lib()
    E, CAP = amd.ORBX_EINVAL, amd.ORBX_ECAP
    assert lib.orbo_create(None) == E
    h = C.c_void_p()
    assert lib.orbo_create(C.byref(h)) == 0 and h.value
    try:
        base = synth.optimize_sim3_problem(1, n=40)
        P, keep = amd.orbo_problem(base)
        R, bufs = amd.Sim3Optimizer._result(P.n)
        assert lib.orbo_optimize_sim3(None, C.byref(P), C.byref(R)) == E
        assert lib.orbo_optimize_sim3(h, None, C.byref(R)) == E
        assert lib.orbo_optimize_sim3(h, C.byref(P), None) == E
        R2, _ = amd.Sim3Optimizer._result(P.n)
        R2.state = None
        assert lib.orbo_optimize_sim3(h, C.byref(P), C.byref(R2)) == E
        assert lib.orbo_reserve(None, 1, 40) == E
        assert lib.orbo_reserve(h, 0, 40) == E and lib.orbo_reserve(h, 1, -1) == E
        assert lib.orbo_stage(h, 0, C.byref(P)) == E             # nothing reserved: no such slot
        assert lib.orbo_run_batch(h, 1, None) == E
        assert lib.orbo_reserve(h, 2, 40) == 0                   # host bookkeeping only
        assert lib.orbo_stage(None, 0, C.byref(P)) == E
        assert lib.orbo_stage(h, 2, C.byref(P)) == E and lib.orbo_stage(h, -1, C.byref(P)) == E
        assert lib.orbo_stage(h, 0, None) == E
        assert lib.orbo_fetch(h, 0, None) == E and lib.orbo_fetch(h, 2, C.byref(R)) == E and lib.orbo_fetch(None, 0, C.byref(R)) == E
        assert lib.orbo_run_batch(h, 3, None) == E and lib.orbo_run_batch(None, 1, None) == E and lib.orbo_run_batch(h, 0, None) == E
        assert lib.orbo_run_batch(h, 1, None) == amd.ORBX_ESTATE  # a slot that was never staged
        assert lib.orbo_fetch(h, 0, C.byref(R)) == amd.ORBX_ESTATE

        def bad(**kw):
            d = dict(base)
            d.update({k: v for k, v in kw.items() if not k.startswith("_")})
            Q, k2 = amd.orbo_problem(d)
            for f, v in kw.items():
                if f.startswith("_"):
                    setattr(Q, f[1:], v)
            return lib.orbo_stage(h, 0, C.byref(Q)), lib.orbo_optimize_sim3(h, C.byref(Q), C.byref(R))

        for f in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
            assert bad(**{"_" + f: None}) == (E, E), f
        assert bad(_n=-1) == (E, E)
        for v in (np.nan, np.inf, -np.inf):
            assert bad(s=v) == (E, E)
            assert bad(q=np.array([0, 0, v, 1.0])) == (E, E)
            assert bad(t=np.array([v, 0, 0.0])) == (E, E)
        assert bad(s=0.0) == (E, E) and bad(s=-1.0) == (E, E)
        big = synth.optimize_sim3_problem(2, n=41)
        Q, k3 = amd.orbo_problem(big)
        assert lib.orbo_stage(h, 0, C.byref(Q)) == CAP           # n > cap_pairs
    finally:
        lib.orbo_destroy(h)


def test_header_declares_orbo_abi():
    """Every orbo_* declaration is bound and exported."""
    import re
    from pathlib import Path
    import orbslam2_amd as amd
    root = Path(__file__).resolve().parents[1]
    text = re.sub(r"/\*.*?\*/", "", (root / "include" / "orbslam2_amd.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(orbo_[a-z0-9_]+)\s*\(", text))
    assert names == {"orbo_create", "orbo_destroy", "orbo_optimize_sim3", "orbo_reserve", "orbo_stage", "orbo_run_batch",
                     "orbo_fetch"}
    assert names <= {n for n, _, _ in amd.SIGNATURES}
    for n in names:
        assert hasattr(amd.lib(), n)
