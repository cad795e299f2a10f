"""bench.py --dump-outputs (no GPU): dump_c2_outputs writes what a caller of the pipeline fetches
(StereoPipeline.fetch / stereo_fetch) as float32 .npy files, for a fixed sample of the batch's pairs
that depends on the arguments only, within the size budget; and the options that belong to a
--full run are refused without it."""
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from orbslam2_amd import KP_DTYPE  # noqa: E402


class FakePipeline:
    """Pair p has 5 + p left and 3 + p right keypoints, every value a function of (p, row)."""

    def __init__(self, nfeatures):
        self.nfeatures = nfeatures
        self.cap = max(64, nfeatures * 2 + 512)

    @staticmethod
    def _image(n, tag):
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"] = np.arange(n) + 0.25, tag
        k["size"], k["angle"], k["response"] = 31.0, 1.5 * np.arange(n), 20 + np.arange(n)
        k["octave"], k["class_id"] = np.arange(n) % 8, -1
        d = ((np.arange(n)[:, None] * 7 + np.arange(32)[None, :] + tag) % 256).astype(np.uint8)
        return k, d

    def fetch(self, p):
        return (*self._image(5 + p, p), *self._image(3 + p, 100 + p))

    def stereo_fetch(self, p):
        u = np.full(self.cap, -1, np.float32)
        d = np.full(self.cap, -1, np.float32)
        u[: 5 + p] = np.arange(5 + p) + 0.5
        d[: 5 + p] = 2.0 + p
        return u, d


def _load(d):
    return {f.stem: np.load(f) for f in sorted(Path(d).glob("*.npy"))}


def test_dump_all_pairs(tmp_path):
    ex = FakePipeline(100)
    bench.dump_c2_outputs(ex, 6, tmp_path / "a")
    a = _load(tmp_path / "a")
    assert sorted(a) == ["counts", "depth", "descriptors_left", "descriptors_right", "keypoints_left",
                         "keypoints_right", "pairs", "u_right"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["pairs"].tolist() == [0, 1, 2, 3, 4, 5]
    assert a["counts"].tolist() == [[5 + p, 3 + p] for p in range(6)]
    nL, nR = sum(5 + p for p in range(6)), sum(3 + p for p in range(6))
    assert a["keypoints_left"].shape == (nL, 7) and a["keypoints_right"].shape == (nR, 7)
    assert a["descriptors_left"].shape == (nL, 32) and a["descriptors_right"].shape == (nR, 32)
    assert a["u_right"].shape == (nL,) and a["depth"].shape == (nL,)
    # pair 2's rows follow pairs 0 and 1's: every field and descriptor byte as fetched
    kL, dL, kR, dR = ex.fetch(2)
    s = 5 + 6
    for j, f in enumerate(KP_DTYPE.names):
        assert np.array_equal(a["keypoints_left"][s:s + 7, j], kL[f].astype(np.float32)), f
    assert np.array_equal(a["descriptors_left"][s:s + 7], dL.astype(np.float32))
    assert np.array_equal(a["descriptors_right"][3 + 4:3 + 4 + 5], dR.astype(np.float32))
    assert np.array_equal(a["depth"][s:s + 7], np.full(7, 4.0, np.float32))


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    ex = FakePipeline(2000)
    per_pair = 2 * ex.cap * (7 + 32) * 4 + 2 * ex.cap * 4 + 3 * 4
    default = bench.DUMP_BUDGET_BYTES
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * per_pair + 1)
    bench.dump_c2_outputs(ex, 384, tmp_path / "a")
    bench.dump_c2_outputs(ex, 384, tmp_path / "b")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    pairs = a["pairs"].astype(int)
    assert len(pairs) == 10 and len(set(pairs)) == 10 and list(pairs) == sorted(pairs) and pairs.max() < 384
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["counts"].tolist() == [[5 + p, 3 + p] for p in pairs]
    # the default budget keeps a dump of full-capacity images (and the 8 .npy headers) under 64 MB
    assert (default // per_pair) * per_pair + 8 * 128 <= 64 * 10**6


def test_full_only_options_refused_without_full():
    for argv, word in ((["--check-parity"], "--full"), (["--steps", "0"], "--steps"),
                       (["--dump-outputs", "x", "--no-c2"], "--no-c2")):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr)
