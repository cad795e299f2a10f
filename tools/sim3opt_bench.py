#!/usr/bin/env python3
"""Optimizer::OptimizeSim3 on the GPU (orbo_run_batch), the shapes of one LoopClosing::ComputeSim3 call:
one launch of 1 x 200 pairs and of 8 x 200 pairs, staged once, timed with device events.

    python3 tools/sim3opt_bench.py [--repeats 300] [--warmup 30] [--out profiles/sim3_optimize.json]

Reports the median and spread of one launch and the LM iterations of both stages per slot. For
context the same run times orbp_run_batch (Optimizer::PoseOptimization) at 8 x 400 edges: existing
code with the same structure (one workgroup per problem, the same LM control and reduction) but an
analytic Jacobian, so a reader can see what g2o's numeric Jacobian -- 2 x 14 extra projections per
pair and linearisation -- costs. No pass / fail threshold is attached to these times. The result is
stamped with the library's source hash (tools/stamp.py)."""
import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "orb-slam2-noted_amd" / "python"))
os.environ.setdefault("ORBSLAM2_AMD_NO_TORCH", "1")   # one HIP runtime in this process: the library's

import orbslam2_amd as amd   # noqa: E402
from orbslam2_amd import synth   # noqa: E402
from stamp import stamp   # noqa: E402

N_PAIRS, N_SLOTS, POSE_EDGES = 200, 8, 400


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


def time_launches(hip, launch, repeats, warmup):
    """Microseconds of `repeats` launches, each between two events on one stream."""
    stream = C.c_void_p()
    chk(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    ev = [(C.c_void_p(), C.c_void_p()) for _ in range(repeats)]
    for e0, e1 in ev:
        chk(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
        chk(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    for _ in range(warmup):
        launch(stream)
    chk(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    for e0, e1 in ev:
        chk(hip.hipEventRecord(e0, stream), "hipEventRecord")
        launch(stream)
        chk(hip.hipEventRecord(e1, stream), "hipEventRecord")
    chk(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    ms = C.c_float()
    us = []
    for e0, e1 in ev:
        chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        us.append(ms.value * 1e3)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    chk(hip.hipStreamDestroy(stream), "hipStreamDestroy")
    us = np.array(us)
    return {"median": float(np.median(us)), "p10": float(np.percentile(us, 10)), "p90": float(np.percentile(us, 90)),
            "min": float(us.min()), "max": float(us.max()), "repeats": repeats, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sim3_optimize.json"))
    a = ap.parse_args()
    if a.repeats < 200:
        raise SystemExit("--repeats must be >= 200")
    if amd.device_count() < 1:
        raise SystemExit("no HIP device")
    hip = hip_runtime()
    probs = [synth.optimize_sim3_problem(900 + c, n=N_PAIRS, fix_scale=True, outlier_frac=0.2) for c in range(N_SLOTS)]
    o = amd.Sim3Optimizer()
    o.reserve(N_SLOTS, N_PAIRS)
    for c, p in enumerate(probs):
        o.stage(c, p)
    t1 = time_launches(hip, lambda st: o.run_batch(1, st), a.repeats, a.warmup)
    t8 = time_launches(hip, lambda st: o.run_batch(N_SLOTS, st), a.repeats, a.warmup)
    res = [o.fetch(c, N_PAIRS) for c in range(N_SLOTS)]
    o.close()
    pose = amd.PoseOptimizer()
    pose.reserve(N_SLOTS, POSE_EDGES)
    for c in range(N_SLOTS):
        pose.stage(c, synth.pose_problem(900 + c, n=POSE_EDGES))
    tp = time_launches(hip, lambda st: pose.run_batch(N_SLOTS, st), a.repeats, a.warmup)
    pres = [pose.fetch(c, POSE_EDGES) for c in range(N_SLOTS)]
    pose.close()
    method = "hipEventRecord before / after each run_batch on one stream, staged once"
    doc = {"stamp": stamp(workload=f"OptimizeSim3: 1 and {N_SLOTS} slots x {N_PAIRS} pairs, fix_scale, 20 % outliers, th2 = 10"),
           "run_batch_1x200_us": dict(t1, method=method), f"run_batch_{N_SLOTS}x200_us": dict(t8, method=method),
           "lm_iterations_per_slot": [list(r["iterations"]) for r in res],
           "n_inliers_per_slot": [int(r["n_inliers"]) for r in res],
           "context_pose_optimization": {f"orbp_run_batch_{N_SLOTS}x{POSE_EDGES}_us": dict(tp, method=method),
                                         "lm_iterations_per_slot": [list(r["iterations"]) for r in pres],
                                         "what": "Optimizer::PoseOptimization, the same launch structure with an analytic "
                                                 "Jacobian: 4 rounds of optimize(10) over 400 unary edges"},
           "note": "no threshold is attached to these times"}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
