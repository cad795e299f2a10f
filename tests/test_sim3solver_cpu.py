"""Sim3Solver without a GPU: the numpy reference (tests/sim3_ref.py) is consistent with itself on
the inputs the GPU tests use, restates SetRansacParameters and the threshold truncation, recovers
the synthetic ground truth, and the orbs_* C-ABI rejects bad arguments before touching a device."""
import ctypes as C

import numpy as np
import pytest

import sim3_ref as ref
from orbslam2_amd import synth


def _names():
    return [f"n{n}-h{h}-fix{f}-k2{int(d)}" for (n, h, f) in ref.CASES for d in (False, True)] + ["hostile"]


def test_reference_modes_agree():
    """float32 (the reference's types) vs float64 on every GPU-test input: identical on decided
    entries, undecided <= 1 % of entries, ill-conditioned <= 2 % of hypotheses (hostile problem: its
    planted triplets aside), the same iterate scan; the measured deviations stay within the constants
    BAND and T_TOL are 4 x of."""
    worst_dev = worst_t = 0.0
    flips = entries = 0
    for name, p in zip(_names(), ref.all_problems()):
        r32, r64 = ref.reference(p, "f32"), ref.reference(p, "f64")
        n, H = len(p["X1c"]), len(p["triplets"])
        dev, tdev = ref.mode_deviation(p, r32, r64)
        wc = ref.well_conditioned(r64)
        dec = ref.decided(p, r64)
        undecided = (~dec & wc[:, None]).sum() / dec.size
        diff = r32["inliers"] != r64["inliers"]
        flips += int(diff.sum())
        entries += diff.size
        print(f"{name}: err dev {dev:.3e}, T dev {tdev:.3e}, undecided {undecided:.4%}, ill {(~wc).sum()}/{H}, "
              f"flips {diff.sum()}")
        worst_dev, worst_t = max(worst_dev, dev), max(worst_t, tdev)
        assert not (diff & dec).any(), name
        assert undecided <= 0.01, name
        if name != "hostile":
            assert (~wc).sum() <= 0.02 * H, name
        s32, s64 = ref.Scan(n, r32["n_inliers"]), ref.Scan(n, r64["n_inliers"])
        a, b = ref.round_robin([s32]), ref.round_robin([s64])
        assert a[:2] == b[:2] and a[3] == b[3], name     # candidate, iteration, the bNoMore pattern
    print(f"largest err dev {worst_dev:.3e} (BAND {ref.BAND:.3e}), largest T dev {worst_t:.3e} (T_TOL {ref.T_TOL:.3e}), "
          f"{flips} flips in {entries} entries")
    assert worst_dev <= ref.MEASURED_ERR_DEV and worst_t <= ref.MEASURED_T_DEV
    assert ref.BAND == 4 * ref.MEASURED_ERR_DEV and ref.T_TOL == 4 * ref.MEASURED_T_DEV


def test_hostile_reference():
    """The planted triplets do what the hostile test relies on, in both modes."""
    p = ref.hostile_problem()
    for mode in ("f32", "f64"):
        r = ref.reference(p, mode)
        assert r["n_inliers"][ref.HOSTILE_COINCIDENT] == 0 and np.isnan(r["R"][ref.HOSTILE_COINCIDENT]).all()
        assert not r["inliers"][:, 20].any() and not r["inliers"][:, 21].any()     # z = 0
    r64 = ref.reference(p, "f64")
    wc = ref.well_conditioned(r64)
    assert not wc[ref.HOSTILE_COINCIDENT] and not wc[ref.HOSTILE_COLLINEAR]
    assert p["behind"].sum() >= 2 and r64["inliers"][:, p["behind"]].any()   # negative depth can be an inlier
    assert r64["n_inliers"].max() > 60


@pytest.mark.parametrize("N,want", [(20, 1), (21, 3), (25, 7), (40, 35), (200, 300), (2000, 300)])
def test_set_ransac_parameters(N, want):
    """mRansacMaxIts of SetRansacParameters(0.99, 20, 300): N = 20 -> 1, else
    ceil(log(0.01) / log(1 - (20 / N)^3)) capped at 300 -- by hand: N = 21: 4.605 / 1.994 = 2.31 -> 3;
    25: 4.605 / 0.7174 = 6.42 -> 7; 40: 4.605 / 0.13353 = 34.49 -> 35; 200: 4603 -> 300; 2000 -> 300."""
    import orbslam2_amd as amd
    assert ref.ransac_iterations(N) == want
    assert amd.Sim3Solver.ransac_iterations(N) == want


def test_too_few_correspondences_is_no_more():
    import orbslam2_amd as amd
    hit, no_more, nin = ref.Scan(10, []).iterate(5)
    assert (hit, no_more, nin) == (-1, True, 0)
    hit, no_more, nin, st = amd.Sim3Solver.iterate([], 5, N=10)
    assert (hit, no_more, nin) == (-1, True, 0)


def test_python_scan_equals_reference_scan():
    """orbslam2_amd.Sim3Solver.iterate replays exactly what the reference scan does, for random counts
    around the threshold and every call size."""
    import orbslam2_amd as amd
    rng = np.random.default_rng(5)
    for trial in range(40):
        N = int(rng.integers(20, 400))
        counts = rng.integers(0, 24, 300)
        if trial % 3 == 0:
            counts[rng.integers(0, 300)] = 30
        sc = ref.Scan(N, counts)
        st = None
        for _ in range(400):
            k = int(rng.integers(1, 8))
            a = sc.iterate(k)
            hit, no_more, nin, st = amd.Sim3Solver.iterate(counts, k, state=st, N=N)
            assert a == (hit, no_more, nin)
            assert st["best"] == sc.best_it
            if no_more or hit >= 0:
                break
        else:
            raise AssertionError("scan did not end")


@pytest.mark.parametrize("k", [6, 7])
def test_reference_recovers_ground_truth(k):
    """The best hypothesis recovers the synthetic Sim3 within the noise (0.4 px lateral at depth,
    0.2 % in depth): rotation within 0.5 deg, translation within 0.1 m, scale within 1 %. A transposed
    M would return the inverse rotation, 2 x the truth's angle (>= 3.9 deg here) away."""
    p = ref.case_problem(k)
    r = ref.reference(p, "f64")
    b = int(r["n_inliers"].argmax())
    Rt = p["R12"]
    truth_angle = np.degrees(np.arccos((np.trace(Rt) - 1) / 2))
    assert truth_angle > 3
    dR = r["R"][b] @ Rt.T
    err = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    assert err < 0.5
    assert np.abs(r["t"][b] - p["t12"]).max() < 0.1
    assert abs(r["s"][b] / p["s12"] - 1) < 0.01
    assert r["n_inliers"][b] > 0.5 * len(p["X1c"])


def test_threshold_truncation():
    """mvnMaxError is a std::vector<size_t>: octave 1 (sigma2 = 1.44) tests against 13, not 13.26."""
    p = synth.sim3_solver_problem(7, n=400)
    want = {0: 9, 1: 13, 2: 19, 3: 27, 4: 39, 5: 57, 6: 82, 7: 118}
    for o, t in want.items():
        assert (p["max_err1"][p["oct1"] == o] == t).all() and (p["oct1"] == o).any()
        assert (p["max_err2"][p["oct2"] == o] == t).all()
    assert p["max_err1"].dtype == np.float32
    # and it matters: an error between 13 and 13.26 is an outlier
    q = ref.case_problem(6)
    r = ref.reference(q, "f64")
    between = (r["err1"] >= q["max_err1"][None, :]) & (r["err1"] < 9.210 * (1.2 ** (2 * q["oct1"]))[None, :])
    assert not (r["inliers"] & between).any()


def test_synth_problem_shape():
    p = synth.sim3_solver_problem(3, n=150, n_hyp=50, fix_scale=False, k2_differs=True)
    t = p["triplets"]
    assert t.shape == (50, 3) and t.min() >= 0 and t.max() < 150
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    assert not np.array_equal(p["K1"], p["K2"]) and p["s12"] != 1.0
    assert p["behind"].any() and (p["X1c"][p["behind"], 2] < 0).all()
    assert 0.15 < p["outlier"].mean() < 0.45
    assert set(np.unique(p["oct1"])) == set(range(8))


def test_orbs_argument_errors_without_gpu():
    """orbs_* return ORBX_EINVAL before touching the device: NULL pointers, n < 3, n_hyp outside
    1..300, n > cap_n, n_hyp > cap_hyp, a triplet index outside [0, n), a repeated index."""
    import orbslam2_amd as amd
    lib = amd.lib()
    E = amd.ORBX_EINVAL
    assert lib.orbs_create(None) == E
    h = C.c_void_p()
    assert lib.orbs_create(C.byref(h)) == 0 and h.value
    try:
        base = synth.sim3_solver_problem(1, n=40, n_hyp=10)
        P, keep = amd.orbs_problem(base)
        R, out = amd.Sim3Solver._result(P.n, P.n_hyp)
        assert lib.orbs_evaluate(None, C.byref(P), C.byref(R)) == E
        assert lib.orbs_evaluate(h, None, C.byref(R)) == E
        assert lib.orbs_evaluate(h, C.byref(P), None) == E
        for f in ("n_inliers", "inlier_bits", "R12", "t12", "s12"):
            R2, _ = amd.Sim3Solver._result(P.n, P.n_hyp)
            setattr(R2, f, None)
            assert lib.orbs_evaluate(h, C.byref(P), C.byref(R2)) == E, f
        assert lib.orbs_reserve(None, 1, 40, 10) == E
        assert lib.orbs_reserve(h, 0, 40, 10) == E
        assert lib.orbs_reserve(h, 1, 2, 10) == E
        assert lib.orbs_reserve(h, 1, 40, 301) == E
        assert lib.orbs_stage(h, 0, C.byref(P)) == E            # nothing reserved: no such slot
        assert lib.orbs_run_batch(h, 1, None) == E
        assert lib.orbs_reserve(h, 2, 40, 10) == 0              # host bookkeeping only
        assert lib.orbs_stage(None, 0, C.byref(P)) == E
        assert lib.orbs_stage(h, 2, C.byref(P)) == E and lib.orbs_stage(h, -1, C.byref(P)) == E
        assert lib.orbs_stage(h, 0, None) == E
        assert lib.orbs_fetch(h, 0, None) == E and lib.orbs_fetch(h, 2, C.byref(R)) == E
        assert lib.orbs_run_batch(h, 3, None) == E and lib.orbs_run_batch(None, 1, None) == E

        def bad(**kw):
            d = dict(base)
            d.update(kw)
            Q, k2 = amd.orbs_problem(d)
            for f, v in kw.items():
                if f.startswith("_"):
                    setattr(Q, f[1:], v)
            return lib.orbs_stage(h, 0, C.byref(Q)), lib.orbs_evaluate(h, C.byref(Q), C.byref(R))

        for f in ("X1c", "X2c", "max_err1", "max_err2", "triplets"):
            assert bad(**{"_" + f: None}) == (E, E), f
        assert bad(_n=2) == (E, E)
        assert bad(_n_hyp=0) == (E, E) and bad(_n_hyp=301) == (E, E)
        t = base["triplets"].copy()
        t[4, 1] = 40
        assert bad(triplets=t) == (E, E)
        t = base["triplets"].copy()
        t[9, 2] = -1
        assert bad(triplets=t) == (E, E)
        t = base["triplets"].copy()
        t[7, 2] = t[7, 0]
        assert bad(triplets=t) == (E, E)
        big = synth.sim3_solver_problem(2, n=41, n_hyp=10)
        Q, k2 = amd.orbs_problem(big)
        assert lib.orbs_stage(h, 0, C.byref(Q)) == E            # n > cap_n
        more = synth.sim3_solver_problem(2, n=40, n_hyp=11)
        Q, k3 = amd.orbs_problem(more)
        assert lib.orbs_stage(h, 0, C.byref(Q)) == E            # n_hyp > cap_hyp
    finally:
        lib.orbs_destroy(h)


def test_header_declares_orbs_abi():
    """Every orbs_* declaration is bound and exported (tests/test_cabi_cpu.py lists other prefixes)."""
    import re
    from pathlib import Path
    import orbslam2_amd as amd
    root = Path(__file__).resolve().parents[1]
    text = re.sub(r"/\*.*?\*/", "", (root / "include" / "orbslam2_amd.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(orbs_[a-z_]+)\s*\(", text))
    assert names == {"orbs_create", "orbs_destroy", "orbs_evaluate", "orbs_reserve", "orbs_stage", "orbs_run_batch",
                     "orbs_fetch"}
    bound = {n for n, _, _ in amd.SIGNATURES}
    assert names <= bound
    assert all(hasattr(amd.lib(), n) for n in names)
