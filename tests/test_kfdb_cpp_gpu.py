"""The C++ host class orbslam2_amd::KeyFrameDatabase (host/orbslam2_amd.hpp) driven from a compiled program
(tests/cpp/kfdb_test.cpp): add with covisibles, SetCovisibles, erase, clear, both queries and Scores give the
candidates and the floats of the CPU restatement tests/kfdb_ref.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kfdb_ref as ref
from orbslam2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "orb-slam2-noted_amd" / "build" / "kfdb_test"


def _bow(w, v):
    return f"{len(w)} " + " ".join(str(int(x)) for x in w) + " " + " ".join(float(x).hex() for x in v)


def _ids(ids):
    return f"{len(ids)} " + " ".join(str(int(i)) for i in ids)


def test_cpp_keyframe_database(amd, tmp_path):
    if not EXE.exists():
        import __graft_entry__
        __graft_entry__.build()
    prob = synth.kfdb_problem(31, n_kf=90, n_words_vocab=700, words_per_kf=(20, 70), n_places=3, n_queries=8)
    db = ref.KeyFrameDatabase(700)
    ops, want = ["700"], []

    def add(k):
        ops.append(f"add {k['id']} {_bow(k['words'], k['values'])} {_ids(k['covisibles'])}")
        db.add(k["id"], k["words"], k["values"])
        db.set_covisibles(k["id"], k["covisibles"])

    def query(q):
        if q["kind"] == ref.LOOP:
            ops.append(f"loop {_bow(q['words'], q['values'])} {_ids(q['connected'])} {float(np.float32(q['min_score'])).hex()}")
            want.append("loop" + "".join(f" {c}" for c in db.query(q)["candidates"]))
        else:
            ops.append(f"reloc {_bow(q['words'], q['values'])}")
            want.append("reloc" + "".join(f" {c}" for c in db.query(q)["candidates"]))

    for k in prob["keyframes"]:
        add(k)
    for q in prob["queries"][:4]:
        query(q)
    for i in (5, 17, 40):
        ops.append(f"erase {i}")
        db.erase(i)
    add(prob["keyframes"][17])
    ops.append(f"cov 3 {_ids([17, 4, 999])}")
    db.set_covisibles(3, [17, 4, 999])
    for q in prob["queries"][4:]:
        query(q)
    q = prob["queries"][0]
    ids = [0, 5, 17, 88]                                   # 5 was erased: skipped
    sc, mn = db.scores(q["words"], q["values"], ids)
    ops.append(f"scores {_bow(q['words'], q['values'])} {_ids(ids)}")
    want.append("scores " + " ".join(float(x).hex() for x in [mn, *sc]))
    ops.append("size")
    want.append("size 88")
    ops += ["clear", "size"]
    want.append("size 0")
    (tmp_path / "in.txt").write_text("\n".join(ops) + "\n")
    r = subprocess.run([str(EXE), "gpu", str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = []
    for line in (tmp_path / "out.txt").read_text().splitlines():
        t = line.split(" ")
        got.append(" ".join([t[0]] + [float.fromhex(x).hex() for x in t[1:]]) if t[0] == "scores" else line)
    assert got == want
    assert sum(len(w.split()) - 1 for w in want[:8]) > 4       # the queries found candidates
