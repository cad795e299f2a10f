"""The front-end test inputs of frontend_cases.py reach what they are built to reach, shown with
the CPU oracle alone: the minThFAST retry supplies a large share of the keypoints, the stereo
disparity window maxD = fx rejects matches, and the disparity <= 0 branch writes outputs. The GPU
tests compare bits on the same inputs; these floors keep a later edit to a generator from turning
them vacuous. The floors are conditions on the inputs, not measurements (measured values in the
comments)."""
import numpy as np
import pytest

import frontend_cases as fc
from orbslam2_amd import synth


def _same(a, b):
    return len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def low_img():
    return fc.low_contrast(synth.textured_image(240, 320, 23))


def test_low_contrast_reaches_the_retry(oracle_mod, low_img):
    """At (20, 7) the retried cells (response < iniThFAST: the cell had no corner at 20) and the
    first-pass cells (response >= 20) both hold >= 100 of the selected keypoints (209 / 179)."""
    k, _ = oracle_mod.Extractor(500, 1.2, 8, 20, 7).extract(low_img)
    lo, hi = int((k["response"] < 20).sum()), int((k["response"] >= 20).sum())
    print("retried", lo, "first pass", hi)
    assert lo >= 100 and hi >= 100


@pytest.mark.parametrize("ini,mn", [(20, 7), (12, 7), (30, 10)])
def test_low_contrast_depends_on_both_thresholds(oracle_mod, low_img, ini, mn):
    """The (ini, min) output differs from (ini, ini) and from (min, min): neither threshold alone
    explains it, so a kernel that mixed them up could not pass."""
    got = oracle_mod.Extractor(500, 1.2, 8, ini, mn).extract(low_img)
    assert not _same(got, oracle_mod.Extractor(500, 1.2, 8, ini, ini).extract(low_img))
    assert not _same(got, oracle_mod.Extractor(500, 1.2, 8, mn, mn).extract(low_img))


@pytest.mark.parametrize("name", list(fc.CAMERAS))
def test_wide_pair_makes_maxd_bind(oracle_mod, name):
    """Disparities up to 1.15 fx: >= 50 matches, >= 20 of them beyond 0.9 fx (next to the window's
    edge), and >= 20 entries of mvuRight change when maxD is four times as wide -- the window
    rejects something. Measured kitti04 / euroc / d435i / small: 369 / 191 / 243 / 98 matches,
    40 / 42 / 21 / 42 beyond 0.9 fx, 98 / 32 / 141 / 68 changed."""
    cam = fc.CAMERAS[name]
    L, R, kL, dL, kR, dR, ((u, d), (u4, d4)) = fc.wide_reference(oracle_mod, name)
    m = u >= 0
    near_edge = int((m & (kL["x"] - u > 0.9 * cam.fx)).sum())
    changed = int((u.view(np.uint32) != u4.view(np.uint32)).sum())
    print(name, "matches", int(m.sum()), "beyond 0.9 fx", near_edge, "changed by maxD x 4", changed)
    assert m.sum() >= 50
    assert near_edge >= 20
    assert changed >= 20


def test_mirror_pair_gives_zero_disparity(oracle_mod):
    """>= 3 matches carry the far depth mbf / 0.01f (9, on octaves 0, 2, 4 and 5) among >= 100
    matches in all (210); each of them has mvuRight = float(double(uL) - 0.01)."""
    L, R = fc.mirror_pair(240, 321, 5)
    kL, dL, kR, dR, ((u, d),) = fc.stereo_reference(oracle_mod, L, R, 500, 20, 7, 386.1448, (0.537,))
    far = d == fc.far_depth(386.1448)
    print("matches", int((u >= 0).sum()), "far", int(far.sum()), "octaves", sorted(set(kL["octave"][far].tolist())))
    assert far.sum() >= 3
    assert (u >= 0).sum() >= 100
    np.testing.assert_array_equal(u[far], (kL["x"][far].astype(np.float64) - 0.01).astype(np.float32))


def test_identical_pair_gives_no_match(oracle_mod):
    """R == L: every SAD is 0, the median is 0 and the cut (Frame.cc:1112-1127) removes every match."""
    L = synth.textured_image(240, 320, 23)
    kL, dL, kR, dR, ((u, d),) = fc.stereo_reference(oracle_mod, L, L, 500, 20, 7, 386.1448, (0.537,))
    assert len(kL) > 100 and (u == -1).all() and (d == -1).all()
