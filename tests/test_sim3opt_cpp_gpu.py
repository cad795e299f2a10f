"""The C++ host layer's Optimizer::OptimizeSim3 / OptimizeSim3All and Sim3 value type
(host/orbslam2_amd.hpp) driven from a compiled C++ program (tests/cpp/optimize_sim3_test.cpp) on a
fixture written here: vpMatches1 with entries the reference skips (Optimizer.cc:1471-1512) between the
real pairs, keyframes at non-identity poses so ToCamera does the P3D1c / P3D2c products. The C++ call
must null exactly the matches the Python binding reports as removed on the compacted problem, write
g2oS12 back byte for byte, and leave it alone on the `return 0` path."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3opt_ref as ref
from orbslam2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "orb-slam2-noted_amd" / "build" / "optimize_sim3_test"


def _read(path, dtypes):
    buf = path.read_bytes()
    out, off = [], 0
    for dt in dtypes:
        n = int(np.frombuffer(buf, np.int64, 1, off)[0])
        off += 8
        out.append(np.frombuffer(buf, dt, n, off).copy())
        off += n * np.dtype(dt).itemsize
    return out


def _to_camera(R, t, Xw):
    """Sim3Solver::ToCamera: one float product and sum at a time."""
    R, t, Xw = R.astype(np.float32), t.astype(np.float32), Xw.astype(np.float32)
    out = np.empty_like(Xw)
    for r in range(3):
        s = R[r, 0] * Xw[:, 0]
        s = s + R[r, 1] * Xw[:, 1]
        s = s + R[r, 2] * Xw[:, 2]
        out[:, r] = s + t[r]
    return out


def _flat(S):
    return np.concatenate([S[0], S[1], [S[2]]])


def test_cpp_optimize_sim3(amd, tmp_path):
    if not EXE.exists():
        import __graft_entry__
        __graft_entry__.build()
    p = synth.optimize_sim3_problem(ref.SEED0 + 70, n=90, fix_scale=False, outlier_frac=0.2, k2_differs=True)
    n = len(p["X1c"])
    rng = np.random.default_rng(17)
    # world points and keyframe poses whose camera-frame products are what ToCamera computes
    R1 = synth._small_rot(rng, 20.0).astype(np.float32)
    R2 = synth._small_rot(rng, 25.0).astype(np.float32)
    t1 = rng.normal(0, 1, 3).astype(np.float32)
    t2 = rng.normal(0, 1, 3).astype(np.float32)
    Xw1 = ((p["X1c"].astype(np.float64) - t1) @ R1.astype(np.float64)).astype(np.float32)
    Xw2 = ((p["X2c"].astype(np.float64) - t2) @ R2.astype(np.float64)).astype(np.float32)
    rows, idx = [], []
    for i in range(n):
        for _ in range(int(rng.integers(0, 3))):                  # entries the reference skips
            kind = int(rng.integers(0, 5))
            flags = [0, 1, 3 | 4, 3 | 8, 3][kind]                 # no match, no pMP1, bad1, bad2, i2 < 0
            rows.append((flags, -1 if kind == 4 else 5, 0, 0, rng.normal(0, 5, 3), rng.normal(0, 5, 3), np.zeros(2), np.zeros(2)))
        idx.append(len(rows))
        rows.append((3, i, int(p["oct1"][i]), int(p["oct2"][i]), Xw1[i], Xw2[i], p["obs1"][i], p["obs2"][i]))
    idx = np.array(idx)
    m = len(rows)
    ints = [np.array([r[c] for r in rows], np.int32) for c in range(4)]
    f32 = [np.array([r[c] for r in rows], np.float32) for c in range(4, 8)]
    S12 = np.concatenate([p["q"], p["t"], [p["s"]]]).astype(np.float64)
    A = (np.array([0.12, -0.05, 0.31, 0.9]), np.array([0.4, -1.5, 2.25]), 1.7)          # not unit: nothing normalises
    B = (np.array([-0.2, 0.44, 0.1, 0.85]), np.array([-3.0, 0.25, 0.5]), 0.6)
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    ang = np.deg2rad(170.0)                                                             # trace < 0: the pivot branch
    Rm = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx) * 1.0000001
    X = np.array([1.5, -2.0, 7.0])
    blob = (np.array([m, 0], np.int32).tobytes() + np.float32(p["th2"]).tobytes() + p["K1"].tobytes() + p["K2"].tobytes() +
            R1.tobytes() + t1.tobytes() + R2.tobytes() + t2.tobytes() + S12.tobytes() + b"".join(a.tobytes() for a in ints) +
            b"".join(a.tobytes() for a in f32) + _flat(A).tobytes() + _flat(B).tobytes() + Rm.astype(np.float64).tobytes() +
            X.tobytes())
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([str(EXE), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    nin, mask, S, mask0, S0, AB, Ainv, AX, SR, Sdef = _read(tmp_path / "out.bin", [np.int32, np.uint8] + [np.float64] + [np.uint8] +
                                                            [np.float64] * 6)
    # the same compacted problem through the Python binding
    q = dict(p)
    q["X1c"], q["X2c"] = _to_camera(R1, t1, Xw1), _to_camera(R2, t2, Xw2)
    o = amd.Sim3Optimizer()
    want = o.optimize(q)
    o.close()
    print(f"C++ OptimizeSim3: nIn {nin[0]} (Python binding {want['n_inliers']}), {int((want['state'] > 0).sum())} of {n} removed, "
          f"{m - n} skipped entries")
    assert want["n_inliers"] >= 20 and (want["state"] == 1).sum() >= 10
    assert nin[0] == nin[1] == nin[2] == want["n_inliers"]
    before = np.array([r[0] & 1 for r in rows], bool)
    after = before.copy()
    after[idx[want["state"] > 0]] = False                          # only real pairs are nulled, through vnIndexEdge
    np.testing.assert_array_equal(mask.astype(bool), after)
    assert S.tobytes() == np.concatenate([want["q"], want["t"], [want["s"]]]).tobytes()
    # th2 = 0: every edge is removed after the first optimize, 0 is returned and g2oS12 is not written
    assert nin[3] == 0 and S0.tobytes() == S12.tobytes()
    after0 = before.copy()
    after0[idx] = False
    np.testing.assert_array_equal(mask0.astype(bool), after0)
    # the value type against the restatement (the same operation sequence in double: a few ulp)
    tol = dict(rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(AB, _flat(ref.sim3_mul(A, B)), **tol)
    np.testing.assert_allclose(Ainv, _flat(ref.sim3_inverse(A)), **tol)
    np.testing.assert_allclose(AX, ref.sim3_map(A, X), **tol)
    assert np.trace(Rm) < 0
    np.testing.assert_allclose(SR, _flat((ref.quat_from_R(Rm), A[1], A[2])), **tol)
    assert abs(np.linalg.norm(SR[:4]) - 1) > 1e-9                  # Sim3(R, t, s) does not normalise
    np.testing.assert_array_equal(Sdef, [0, 0, 0, 1, 0, 0, 0, 1])
