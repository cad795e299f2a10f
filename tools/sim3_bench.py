#!/usr/bin/env python3
"""Sim3Solver hypothesis evaluation, the shape of one LoopClosing::ComputeSim3 call: 8 candidates x
300 hypotheses x 200 correspondences, staged once, orbs_run_batch timed with device events.

    python3 tools/sim3_bench.py [--repeats 300] [--warmup 30] [--out profiles/sim3_solver.json]

Reports the median and spread of one launch (all 2400 hypotheses) and, for context, the wall time of
one whole round-robin through the drop-in C++ class (tests/cpp/sim3_solver_test.cpp: EvaluateAll =
draw + stage + launch + fetch, then the iterate(5) scan) on the same inputs, after a warm-up call. The
numpy reference of tests/sim3_ref.py is not timed: it is a checker, not a fair CPU baseline. The
result is stamped with the library's source hash (tools/stamp.py)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "orb-slam2-noted_amd" / "python"))
os.environ.setdefault("ORBSLAM2_AMD_NO_TORCH", "1")   # one HIP runtime in this process: the library's

import orbslam2_amd as amd   # noqa: E402
from orbslam2_amd import synth   # noqa: E402
from stamp import stamp   # noqa: E402

N_CAND, N_HYP, N_CORR = 8, 300, 200
EXE = ROOT / "orb-slam2-noted_amd" / "build" / "sim3_solver_test"


def hip_runtime():
    """The libamdhip64 the library itself loaded (events must come from the same runtime)."""
    amd.lib()
    for line in Path("/proc/self/maps").read_text().splitlines():
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("libamdhip64 is not loaded")


def chk(rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed with HIP error {rc}")


def host_round_robin(probs):
    """Wall microseconds of EvaluateAll + the iterate(5) round-robin in the C++ class, third call."""
    blob = [np.int32(len(probs)).tobytes()]
    for p in probs:
        n = len(p["X1c"])
        idx = np.arange(n, dtype=np.int32)
        blob += [np.array([n, 1 if p["fix_scale"] else 0], np.int32).tobytes(), np.asarray(p["K1"], np.float32).tobytes(),
                 np.asarray(p["K2"], np.float32).tobytes(), np.full(n, 3, np.int32).tobytes(), idx.tobytes(), idx.tobytes(),
                 p["oct1"].astype(np.int32).tobytes(), p["oct2"].astype(np.int32).tobytes(),
                 p["X1c"].astype(np.float32).tobytes(), p["X2c"].astype(np.float32).tobytes()]
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "in.bin").write_bytes(b"".join(blob))
        subprocess.run([str(EXE), f"{d}/in.bin", f"{d}/out.bin", "1", "3"], check=True, timeout=120)
        buf = (Path(d) / "out.bin").read_bytes()
    n = int(np.frombuffer(buf, np.int64, 1, 0)[0])
    winner, hit, nin, calls, us = (int(v) for v in np.frombuffer(buf, np.int32, n, 8))
    return {"wall_us": us, "winner": winner, "iteration": hit, "n_inliers": nin, "iterate_calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sim3_solver.json"))
    a = ap.parse_args()
    if a.repeats < 200:
        raise SystemExit("--repeats must be >= 200")
    if amd.device_count() < 1:
        raise SystemExit("no HIP device")
    probs = [synth.sim3_solver_problem(700 + c, n=N_CORR, n_hyp=N_HYP, fix_scale=True, outlier_frac=0.3) for c in range(N_CAND)]
    s = amd.Sim3Solver()
    s.reserve(N_CAND, N_CORR, N_HYP)
    for c, p in enumerate(probs):
        s.stage(c, p)
    hip = hip_runtime()
    stream = C.c_void_p()
    chk(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    ev = [(C.c_void_p(), C.c_void_p()) for _ in range(a.repeats)]
    for e0, e1 in ev:
        chk(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
        chk(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    for _ in range(a.warmup):
        s.run_batch(N_CAND, stream)
    chk(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    for e0, e1 in ev:
        chk(hip.hipEventRecord(e0, stream), "hipEventRecord")
        s.run_batch(N_CAND, stream)
        chk(hip.hipEventRecord(e1, stream), "hipEventRecord")
    chk(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    ms = C.c_float()
    us = []
    for e0, e1 in ev:
        chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        us.append(ms.value * 1e3)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    us = np.array(us)
    counts = [int(s.fetch(c, N_CORR, N_HYP)["n_inliers"].max()) for c in range(N_CAND)]
    chk(hip.hipStreamDestroy(stream), "hipStreamDestroy")
    s.close()
    doc = {"stamp": stamp(workload=f"{N_CAND} candidates x {N_HYP} hypotheses x {N_CORR} correspondences, fix_scale"),
           "run_batch_us": {"median": float(np.median(us)), "p10": float(np.percentile(us, 10)),
                            "p90": float(np.percentile(us, 90)), "min": float(us.min()), "max": float(us.max()),
                            "repeats": a.repeats, "warmup": a.warmup,
                            "method": "hipEventRecord before / after each orbs_run_batch on one stream, staged once"},
           "hypotheses_per_launch": N_CAND * N_HYP, "best_inliers_per_candidate": counts,
           "host_round_robin": dict(host_round_robin(probs),
                                    what="C++ Sim3Solver::EvaluateAll (draw, stage, launch, fetch) + iterate(5) round-robin, "
                                         "third call of the process, wall clock"),
           "note": "the numpy reference (tests/sim3_ref.py) is a checker and is not a CPU baseline"}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
