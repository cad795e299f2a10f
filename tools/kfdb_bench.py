#!/usr/bin/env python3
"""KeyFrameDatabase queries at the size of a long KITTI sequence: 2000 keyframes of about 1500 words each in
a 10^6-word vocabulary; one relocalisation query, and one batch of 64 queries, each timed with device events
around orbd_run_batch (one upload of the queries' records, the four kernels, one copy of the results to
page-locked memory).

    python3 tools/kfdb_bench.py [--repeats 300] [--warmup 30] [--out profiles/kfdb_query.json]

Also reported: the bytes the score kernel reads per query (every stored BowVector once: 12 bytes per word)
against the measured HBM copy rate of the part, 6.29 TB/s. The Python restatement tests/kfdb_ref.py is a
checker, not a CPU baseline, and is not timed. The result is stamped with the library's source hash."""
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

N_KF, N_WORDS, WORDS = 2000, 1_000_000, (1400, 1600)
BATCH = 64
HBM_TBS = 6.29   # measured float4 copy rate of the MI355X


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


def timed(hip, stream, db, n_slots, repeats, warmup):
    ev = [(C.c_void_p(), C.c_void_p()) for _ in range(repeats)]
    for e0, e1 in ev:
        chk(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
        chk(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    for _ in range(warmup):
        db.run_batch(n_slots, stream)
    db.fetch(0)
    for e0, e1 in ev:
        chk(hip.hipEventRecord(e0, stream), "hipEventRecord")
        db.run_batch(n_slots, stream)
        chk(hip.hipEventRecord(e1, stream), "hipEventRecord")
    chk(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    ms, us = C.c_float(), []
    for e0, e1 in ev:
        chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        us.append(ms.value * 1e3)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    us = np.array(us)
    return {"median": float(np.median(us)), "p10": float(np.percentile(us, 10)), "p90": float(np.percentile(us, 90)),
            "min": float(us.min()), "max": float(us.max()), "repeats": repeats, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kfdb_query.json"))
    a = ap.parse_args()
    if a.repeats < 200:
        raise SystemExit("--repeats must be >= 200")
    if amd.device_count() < 1:
        raise SystemExit("no HIP device")
    prob = synth.kfdb_problem(77, n_kf=N_KF, n_words_vocab=N_WORDS, words_per_kf=WORDS, n_places=40, overlap=0.6,
                              n_queries=BATCH)
    db = amd.KeyFrameDatabase(N_WORDS)
    stored = 0
    for k in prob["keyframes"]:
        db.add(k["id"], k["words"], k["values"])
        stored += len(k["words"])
    for k in prob["keyframes"]:
        db.set_covisibles(k["id"], k["covisibles"])
    hip = hip_runtime()
    stream = C.c_void_p()
    chk(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    db.reserve(BATCH)
    reloc = [dict(q, kind=amd.ORBD_RELOC) for q in prob["queries"]]
    for s, q in enumerate(reloc):
        db.stage(s, q)
    one = timed(hip, stream, db, 1, a.repeats, a.warmup)
    first = db.fetch(0)
    for s, q in enumerate(prob["queries"]):     # the batch: relocalisation and loop queries alternate
        db.stage(s, q)
    batch = timed(hip, stream, db, BATCH, a.repeats, a.warmup)
    cands = [len(db.fetch(s)["candidates"]) for s in range(BATCH)]
    chk(hip.hipStreamDestroy(stream), "hipStreamDestroy")
    db.close()
    bytes_per_query = 12 * stored
    floor_us = bytes_per_query / (HBM_TBS * 1e12) * 1e6

    def with_rate(t, nq):
        return dict(t, us_per_query=t["median"] / nq, effective_TBps=bytes_per_query * nq / (t["median"] * 1e-6) / 1e12)
    doc = {"stamp": stamp(workload=f"{N_KF} keyframes x {WORDS[0]}-{WORDS[1]} words, {N_WORDS} word vocabulary"),
           "method": "hipEventRecord before / after each orbd_run_batch on one stream, staged once: one upload, "
                     "kfdb_score / select / groups / state kernels, one download to page-locked memory",
           "one_reloc_query_us": with_rate(one, 1), "batch_of_64_us": with_rate(batch, BATCH),
           "stored_words": stored, "bytes_read_per_query": bytes_per_query,
           "hbm_floor_us_per_query": floor_us, "hbm_rate_TBps": HBM_TBS,
           "scored_first_query": int(len(first["scored_ids"])), "candidates_per_batch_slot": cands,
           "note": "effective_TBps counts every stored BowVector as read once per query; a batch re-reads them from "
                   "cache, so it may exceed the HBM rate. tests/kfdb_ref.py is a checker, not a CPU baseline"}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
