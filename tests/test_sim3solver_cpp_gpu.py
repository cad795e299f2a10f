"""The C++ host class orbslam2_amd::Sim3Solver (host/orbslam2_amd.hpp) driven from a compiled C++
program (tests/cpp/sim3_solver_test.cpp): EvaluateAll over 3 candidates, then LoopClosing::ComputeSim3's
round-robin of iterate(5). An injected generator makes the run deterministic, so the candidate that
succeeds, its iteration and nInliers must equal the Python replay on the same triplets."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from orbslam2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "orb-slam2-noted_amd" / "build" / "sim3_solver_test"
SEED = 29


def _read(path, dtypes):
    buf = path.read_bytes()
    out, off = [], 0
    for dt in dtypes:
        n = int(np.frombuffer(buf, np.int64, 1, off)[0])
        off += 8
        out.append(np.frombuffer(buf, dt, n, off).copy())
        off += n * np.dtype(dt).itemsize
    return out


class Lcg:
    """The generator sim3_solver_test.cpp injects."""

    def __init__(self, seed):
        self.state = seed & 0xFFFFFFFF

    def random_int(self, lo, hi):
        self.state = (self.state * 1103515245 + 12345) & 0x7FFFFFFF
        return lo + (self.state >> 8) % (hi - lo + 1)


def draw_triplets(rnd, n, its):
    """Sim3Solver.cc:240-261: three draws with swap-with-back removal, per iteration."""
    out = []
    for _ in range(its):
        avail = list(range(n))
        for _ in range(3):
            r = rnd.random_int(0, len(avail) - 1)
            out.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
    return np.array(out, np.int32).reshape(-1, 3)


def candidate_blob(p, rng):
    """vpMatched12 with gaps around the problem's correspondences: entries the constructor skips
    (NULL on either side, bad points, index < 0) in between. -> (bytes, mvnIndices1, mN1)."""
    n = len(p["X1c"])
    rows, idx = [], []
    for i in range(n):
        for _ in range(int(rng.integers(0, 3))):
            kind = int(rng.integers(0, 6))
            flags = [0, 1, 2, 3 | 4, 3 | 8, 3][kind]
            i1, i2 = (-1, 4) if kind == 5 else (3, 5)
            rows.append((flags, i1, i2, 0, 0, rng.normal(0, 5, 3), rng.normal(0, 5, 3)))
        idx.append(len(rows))
        rows.append((3, i, i, int(p["oct1"][i]), int(p["oct2"][i]), p["X1c"][i], p["X2c"][i]))
    m = len(rows)
    cols = [np.array([r[c] for r in rows], np.int32) for c in range(5)]
    X1 = np.array([r[5] for r in rows], np.float32)
    X2 = np.array([r[6] for r in rows], np.float32)
    blob = (np.array([m, 1 if p["fix_scale"] else 0], np.int32).tobytes() + np.asarray(p["K1"], np.float32).tobytes() +
            np.asarray(p["K2"], np.float32).tobytes() + b"".join(c.tobytes() for c in cols) + X1.tobytes() + X2.tobytes())
    return blob, np.array(idx), m


def test_cpp_sim3solver_round_robin(amd, tmp_path):
    if not EXE.exists():
        import __graft_entry__
        __graft_entry__.build()
    cands = [synth.sim3_solver_problem(901, n=12, n_hyp=1),                                   # N < 20: bNoMore at once
             synth.sim3_solver_problem(902, n=100, n_hyp=1, outlier_frac=0.92),               # never enough inliers
             synth.sim3_solver_problem(903, n=80, n_hyp=1, outlier_frac=0.55, k2_differs=True)]
    rng = np.random.default_rng(9)
    blobs = [candidate_blob(p, rng) for p in cands]
    (tmp_path / "in.bin").write_bytes(np.int32(len(cands)).tobytes() + b"".join(b[0] for b in blobs))
    r = subprocess.run([str(EXE), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(SEED)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    summary, per, trips, inl8, T12, Rts, thr0 = _read(tmp_path / "out.bin", [np.int32, np.int32, np.int32, np.uint8,
                                                                             np.float32, np.float32, np.int32])
    winner, hit, nin, calls, _us = (int(v) for v in summary)
    per = per.reshape(len(cands), 3)
    # constructor: compaction and the truncated thresholds
    np.testing.assert_array_equal(per[:, 0], [len(p["X1c"]) for p in cands])
    np.testing.assert_array_equal(thr0, cands[0]["max_err1"].astype(np.int32))
    np.testing.assert_array_equal(per[:, 1], [amd.Sim3Solver.ransac_iterations(len(p["X1c"])) if len(p["X1c"]) >= 20 else 300
                                              for p in cands])
    # the injected generator: the solvers with N >= mRansacMinInliers draw all their triplets up front, in order
    rnd = Lcg(SEED)
    want_trips = [draw_triplets(rnd, len(p["X1c"]), int(per[c, 1])) for c, p in enumerate(cands) if len(p["X1c"]) >= 20]
    np.testing.assert_array_equal(trips.reshape(-1, 3), np.concatenate(want_trips))
    # Python replay on the same triplets
    s = amd.Sim3Solver()
    outs, states = [None], [None]
    for p, t in zip(cands[1:], want_trips):
        q = dict(p)
        q["triplets"] = t
        outs.append(s.evaluate(q))
        states.append(None)
    alive = [True] * len(cands)
    py_calls, py_winner, py_hit, py_nin = 0, -1, -1, 0
    while any(alive) and py_winner < 0:
        for c, p in enumerate(cands):
            if not alive[c] or py_winner >= 0:
                continue
            counts = outs[c]["n_inliers"] if outs[c] is not None else []
            h, no_more, n_in, states[c] = amd.Sim3Solver.iterate(counts, 5, state=states[c], N=len(p["X1c"]))
            py_calls += 1
            if no_more:
                alive[c] = False
            if h >= 0:
                py_winner, py_hit, py_nin = c, h, n_in
    print(f"C++: candidate {winner}, iteration {hit}, {nin} inliers after {calls} iterate() calls; Python replay: "
          f"{py_winner}, {py_hit}, {py_nin}, {py_calls}")
    assert py_winner == 2 and py_calls > 3, "the scenario should take several rounds and end at the last candidate"
    assert (winner, hit, nin, calls) == (py_winner, py_hit, py_nin, py_calls)
    assert per[winner, 2] == hit + 1 and per[0, 2] == 0
    o = outs[winner]
    n = len(cands[winner]["X1c"])
    vb = np.zeros(blobs[winner][2], bool)
    vb[blobs[winner][1]] = amd.Sim3Solver.unpack_bits(o["inlier_bits"], n)[hit]
    np.testing.assert_array_equal(inl8.astype(bool), vb)                 # vbInliers: size mN1, through mvnIndices1
    assert Rts[:9].tobytes() == o["R12"][hit].tobytes() and Rts[9:12].tobytes() == o["t12"][hit].tobytes()
    assert Rts[12] == o["s12"][hit]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = o["s12"][hit] * o["R12"][hit]
    T[:3, 3] = o["t12"][hit]
    assert T12.tobytes() == T.tobytes()
    s.close()
