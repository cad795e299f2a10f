"""GPU parity of Frame::ComputeStereoMatches (Frame.cc:831-1128) and the Hamming core
(ORBmatcher.cc:2123-2143) against the CPU oracle: mvuRight / mvDepth bit-exact."""
import numpy as np
import pytest

import frontend_cases as fc
from orbslam2_amd import synth

pytestmark = pytest.mark.gpu

KITTI_BF = 386.1448       # Stereo/KITTI00-02.yaml:25 (Camera.bf)
KITTI_FX = 718.856        # Stereo/KITTI00-02.yaml:8


def _stereo_ref(oracle_mod, L, R, nf):
    exL = oracle_mod.Extractor(nf, 1.2, 8, 20, 7)
    exR = oracle_mod.Extractor(nf, 1.2, 8, 20, 7)
    kL, dL = exL.extract(L)
    kR, dR = exR.extract(R)
    mb = np.float32(KITTI_BF) / np.float32(KITTI_FX)
    u, d = oracle_mod.stereo_matches(exL, exR, kL, dL, kR, dR, KITTI_BF, float(mb))
    return kL, u, d, float(mb)


@pytest.mark.parametrize("t", [0, 3])
def test_stereo_single_pair(amd, oracle_mod, t):
    L, R = synth.stereo_pair(376, 1241, t)
    kL, u_ref, d_ref, mb = _stereo_ref(oracle_mod, L, R, 2000)
    exL = amd.ORBextractor(2000)
    exR = amd.ORBextractor(2000)
    k, _ = exL(L)
    exR(R)
    assert len(k) == len(kL)
    u, d = amd.compute_stereo_matches(exL, exR, len(k), KITTI_BF, mb)
    assert (u_ref >= 0).sum() > 100, "synthetic pair should produce stereo matches"
    np.testing.assert_array_equal(u.view(np.uint32), u_ref.view(np.uint32))
    np.testing.assert_array_equal(d.view(np.uint32), d_ref.view(np.uint32))


@pytest.mark.parametrize("nf", [90, 300])
def test_stereo_few_features(amd, oracle_mod, nf):
    """Keypoint counts that leave the last staged workgroup (32 left keypoints, 8 per wavefront)
    partly filled, and images with few candidates per band."""
    L, R = synth.stereo_pair(376, 1241, 5)
    kL, u_ref, d_ref, mb = _stereo_ref(oracle_mod, L, R, nf)
    exL = amd.ORBextractor(nf)
    exR = amd.ORBextractor(nf)
    k, _ = exL(L)
    exR(R)
    assert len(k) == len(kL)
    u, d = amd.compute_stereo_matches(exL, exR, len(k), KITTI_BF, mb)
    np.testing.assert_array_equal(u.view(np.uint32), u_ref.view(np.uint32))
    np.testing.assert_array_equal(d.view(np.uint32), d_ref.view(np.uint32))


@pytest.mark.parametrize("rows", [36, 160])
def test_stereo_dense_rows(amd, oracle_mod, rows):
    """Keypoints packed into a band of rows: with 36 rows every candidate band holds far more
    right keypoints than a workgroup stages (ST_SCAP, orb_stereo.hip), so the staged matcher
    takes its global-memory scan; with 160 rows both forms occur."""
    h, w = 376, 1241
    rng = np.random.default_rng(rows)
    L = np.full((h, w), 40, np.uint8)
    y0 = (h - rows) // 2
    L[y0:y0 + rows] = rng.integers(0, 256, size=(rows, w), dtype=np.uint8)
    R = np.roll(L, -17, axis=1)
    R[:, -17:] = 40
    kL, u_ref, d_ref, mb = _stereo_ref(oracle_mod, L, R, 2000)
    exL = amd.ORBextractor(2000)
    exR = amd.ORBextractor(2000)
    k, _ = exL(L)
    exR(R)
    assert len(k) == len(kL)
    u, d = amd.compute_stereo_matches(exL, exR, len(k), KITTI_BF, mb)
    assert (u_ref >= 0).sum() > 50
    np.testing.assert_array_equal(u.view(np.uint32), u_ref.view(np.uint32))
    np.testing.assert_array_equal(d.view(np.uint32), d_ref.view(np.uint32))


def test_stereo_batch(amd, oracle_mod):
    import torch
    h, w, P = 376, 1241, 3
    pairs = [synth.stereo_pair(h, w, 10 + p) for p in range(P)]
    imgs = np.stack([im for pr in pairs for im in pr])
    dev = torch.from_numpy(imgs).cuda()
    ex = amd.BatchExtractor(2000)
    ex.reserve(w, h, 2 * P)
    torch.cuda.synchronize()
    ex.extract_device(dev.data_ptr(), 2 * P, w, h, w, h * w)
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    ex.stereo_batch(P, KITTI_BF, mb)
    for p in range(P):
        kL, u_ref, d_ref, _ = _stereo_ref(oracle_mod, *pairs[p], 2000)
        u, d = ex.stereo_fetch(p)
        n = len(kL)
        np.testing.assert_array_equal(u[:n].view(np.uint32), u_ref.view(np.uint32))
        np.testing.assert_array_equal(d[:n].view(np.uint32), d_ref.view(np.uint32))


def test_hamming_best2(amd, oracle_mod):
    rng = np.random.default_rng(3)
    db = rng.integers(0, 256, size=(1500, 32), dtype=np.uint8)
    q = db[rng.integers(0, 1500, 300)].copy()
    q[::2, 0] ^= 0x5A  # near-duplicates and exact duplicates
    dbd = np.concatenate([db, db[:50]])  # duplicate rows -> ties resolved to first index
    bi, bd, sd = amd.ORBmatcher.hamming_best2(q, dbd)
    ri, rd, rs = oracle_mod.hamming_best2(q, dbd)
    np.testing.assert_array_equal(bi, ri)
    np.testing.assert_array_equal(bd, rd)
    np.testing.assert_array_equal(sd, rs)


@pytest.mark.parametrize("P,k", [(5, 3), (2, 3), (4, 2)])
def test_stereo_pipeline(amd, oracle_mod, P, k):
    """orbx_pipeline_*: k engines on k streams, chunks of consecutive pairs (uneven and empty
    chunks included), two batches back to back (the second's phase 1 waits on the first's),
    every pair bit-exact with the oracle's extraction + ComputeStereoMatches."""
    import torch
    h, w = 376, 1241
    pairs = [synth.stereo_pair(h, w, 20 + p) for p in range(P)]
    imgs = np.stack([im for pr in pairs for im in pr])
    dev = torch.from_numpy(imgs).cuda()
    dev2 = torch.flip(dev, dims=[0]).contiguous()   # second batch: pairs reversed, L / R swapped
    pl = amd.StereoPipeline(2000, n_engines=k)
    pl.reserve(w, h, P)
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    torch.cuda.synchronize()
    pl.stereo_batch(dev2.data_ptr(), P, w, h, w, h * w, KITTI_BF, mb)
    pl.stereo_batch(dev.data_ptr(), P, w, h, w, h * w, KITTI_BF, mb)
    torch.cuda.synchronize()
    assert sum(pl.chunk(i)[2] for i in range(k)) == P
    for p in range(P):
        kL, u_ref, d_ref, _ = _stereo_ref(oracle_mod, *pairs[p], 2000)
        gkL, gdL, gkR, gdR = pl.fetch(p)
        assert gkL.tobytes() == kL.tobytes()
        u, d = pl.stereo_fetch(p)
        n = len(kL)
        np.testing.assert_array_equal(u[:n].view(np.uint32), u_ref.view(np.uint32))
        np.testing.assert_array_equal(d[:n].view(np.uint32), d_ref.view(np.uint32))
    pl.close()


def test_stereo_pipeline_opencv32(amd, oracle_mod):
    """The pipeline under the reference's documented platform (OpenCV 3.2 on x86-64, README.md:9):
    the SSE2 resize layout (resize_mode 1) and the half-even GaussianBlur column pass (blur_mode 1),
    12 pairs over 3 engines: keypoints, descriptors, mvuRight and mvDepth bit-exact against the
    oracle in the same variants."""
    import torch
    h, w, P, k = 376, 1241, 12, 3
    pairs = [synth.stereo_pair(h, w, 50 + p) for p in range(P)]
    dev = torch.from_numpy(np.stack([im for pr in pairs for im in pr])).cuda()
    pl = amd.StereoPipeline(2000, n_engines=k, resize_mode=1, blur_mode=1)
    pl.reserve(w, h, P)
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    torch.cuda.synchronize()
    pl.stereo_batch(dev.data_ptr(), P, w, h, w, h * w, KITTI_BF, mb)
    torch.cuda.synchronize()
    for p in range(P):
        L, R = pairs[p]
        exL = oracle_mod.Extractor(2000, resize_mode=1, blur_mode=1)
        exR = oracle_mod.Extractor(2000, resize_mode=1, blur_mode=1)
        kL, dL = exL.extract(L)
        kR, dR = exR.extract(R)
        u, d = oracle_mod.stereo_matches(exL, exR, kL, dL, kR, dR, KITTI_BF, mb)
        _check_pair((*pl.fetch(p), *[a[:len(kL)] for a in pl.stereo_fetch(p)]), (kL, dL, kR, dR, u, d), f"pair {p}")
    pl.close()


def test_stereo_pipeline_host_mode(amd, oracle_mod):
    """orbx_pipeline_stereo_batch_host: host (pinned) images in, host outputs out, the H2D of the
    next batch overlapping the current one, three batches back to back into two output buffers
    (two device input slots): every pair bit-exact with the oracle."""
    h, w, P, k = 376, 1241, 7, 3
    pairs = [synth.stereo_pair(h, w, 40 + p) for p in range(P)]
    ins = []
    for b in range(3):
        a = amd.host_empty((2 * P, h, w), np.uint8)
        for p in range(P):
            L, R = pairs[(p + b) % P]
            a[2 * p], a[2 * p + 1] = L, R
        ins.append(a)
    pl = amd.StereoPipeline(2000, n_engines=k)
    pl.reserve(w, h, P)
    cap = pl.capacity()
    outs = [amd.StereoHostBatch(P, cap), amd.StereoHostBatch(P, cap)]
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    refs = [_stereo_ref_full(oracle_mod, *pairs[p]) for p in range(P)]
    pl.stereo_batch_host(ins[0], P, w, h, w, w * h, KITTI_BF, mb, outs[0])
    pl.stereo_batch_host(ins[1], P, w, h, w, w * h, KITTI_BF, mb, outs[1])
    pl.wait()
    got1 = [outs[1].pair(p) for p in range(P)]
    got1 = [tuple(np.array(x) for x in g) for g in got1]
    for b, out in ((0, outs[0]),):
        for p in range(P):
            _check_pair(out.pair(p), refs[(p + b) % P], f"batch {b} pair {p}")
    pl.stereo_batch_host(ins[2], P, w, h, w, w * h, KITTI_BF, mb, outs[0])
    pl.wait()
    for p in range(P):
        _check_pair(got1[p], refs[(p + 1) % P], f"batch 1 pair {p}")
        _check_pair(outs[0].pair(p), refs[(p + 2) % P], f"batch 2 pair {p}")
    pl.close()


def _stereo_ref_full(oracle_mod, L, R):
    exL, exR = oracle_mod.Extractor(2000), oracle_mod.Extractor(2000)
    kL, dL = exL.extract(L)
    kR, dR = exR.extract(R)
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    u, d = oracle_mod.stereo_matches(exL, exR, kL, dL, kR, dR, KITTI_BF, mb)
    return kL, dL, kR, dR, u, d


def _check_pair(got, ref, what):
    gkL, gdL, gkR, gdR, gu, gd = got
    kL, dL, kR, dR, u, d = ref
    assert gkL.tobytes() == kL.tobytes() and np.array_equal(gdL, dL), what + " left"
    assert gkR.tobytes() == kR.tobytes() and np.array_equal(gdR, dR), what + " right"
    assert gu.tobytes() == u.tobytes() and gd.tobytes() == d.tobytes(), what + " stereo"


def test_stereo_pipeline_host_mode_varying_stride(amd, oracle_mod):
    """host-mode batches (10 pairs, stride S), (5, S), (10, S), (5, 2S) -- slot 1 is reused
    with the same pair count but a larger image stride while it is already big enough, so chunk j's
    upload covers byte ranges that engines j+1.. read in slot 1's previous batch: the upload must wait
    for every engine's reads, not only engines 0..j (the layout is keyed on count and stride)."""
    h, w, k = 376, 1241, 3
    S = w * h
    pairs = [synth.stereo_pair(h, w, 80 + p) for p in range(10)]
    refs = [_stereo_ref_full(oracle_mod, *pr) for pr in pairs]
    plan = ((10, 1), (5, 1), (10, 1), (5, 2))   # (pairs, stride in images)
    order = [[(p * 7 + b) % 10 for p in range(P)] for b, (P, _) in enumerate(plan)]
    ins = []
    for b, (P, m) in enumerate(plan):
        a = amd.host_empty((2 * P, m * h, w), np.uint8)
        a[...] = 0xA5                             # the gap rows of the wide stride are never read
        for p, q in enumerate(order[b]):
            a[2 * p, :h], a[2 * p + 1, :h] = pairs[q]
        ins.append(a)
    pl = amd.StereoPipeline(2000, n_engines=k)
    pl.reserve(w, h, 10)
    cap = pl.capacity()
    outs = [amd.StereoHostBatch(P, cap) for P, _ in plan]
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    for b, (P, m) in enumerate(plan):
        pl.stereo_batch_host(ins[b], P, w, h, w, m * S, KITTI_BF, mb, outs[b])
    pl.wait()
    for b, (P, _) in enumerate(plan):
        for p, q in enumerate(order[b]):
            _check_pair(outs[b].pair(p), refs[q], f"batch {b} pair {p}")
    pl.close()


def test_stereo_pipeline_host_mode_varying_batches(amd, oracle_mod):
    """Host-mode batches of 10, 5 and 8 pairs (slot 0, slot 1, slot 0 again): the third batch's
    chunk ranges in slot 0 straddle the first batch's, so its uploads must wait for every engine's
    reads of the first batch, not only engines 0..j. Then a device-input batch is enqueued before
    wait(): its phase 2 must not overwrite outputs still draining to the host."""
    import torch
    h, w, k = 376, 1241, 3
    pairs = [synth.stereo_pair(h, w, 60 + p) for p in range(10)]
    refs = [_stereo_ref_full(oracle_mod, *pr) for pr in pairs]
    sizes = (10, 5, 8)
    order = [[(p * 3 + b) % 10 for p in range(P)] for b, P in enumerate(sizes)]
    ins = []
    for b, P in enumerate(sizes):
        a = amd.host_empty((2 * P, h, w), np.uint8)
        for p, q in enumerate(order[b]):
            a[2 * p], a[2 * p + 1] = pairs[q]
        ins.append(a)
    pl = amd.StereoPipeline(2000, n_engines=k)
    pl.reserve(w, h, 10)
    cap = pl.capacity()
    outs = [amd.StereoHostBatch(P, cap) for P in sizes]
    with pytest.raises(ValueError):
        pl.stereo_batch_host(ins[0], 10, w, h, w, w * h, KITTI_BF, 0.5, amd.StereoHostBatch(4, cap))
    mb = float(np.float32(KITTI_BF) / np.float32(KITTI_FX))
    for b, P in enumerate(sizes):
        pl.stereo_batch_host(ins[b], P, w, h, w, w * h, KITTI_BF, mb, outs[b])
    dev = torch.from_numpy(np.flip(ins[0], axis=0).copy()).cuda()   # reversed: other content per engine
    torch.cuda.synchronize()
    pl.stereo_batch(dev.data_ptr(), 10, w, h, w, h * w, KITTI_BF, mb)
    pl.wait()
    for b, P in enumerate(sizes):
        for p, q in enumerate(order[b]):
            _check_pair(outs[b].pair(p), refs[q], f"batch {b} pair {p}")
    torch.cuda.synchronize()
    pl.close()


# ---- the shipped cameras, a binding disparity window, zero disparity (inputs: frontend_cases.py,
# pinned with the oracle alone by test_frontend_cases_cpu.py). All through the two-engine drop-in
# path ORBextractor x 2 + compute_stereo_matches.

def _drop_in(amd, L, R, nf, ini, mn, ref, what):
    """Two engines on L and R; their keypoints and descriptors must equal the oracle's (kL, dL, kR,
    dR = ref[:4]) before any stereo compare, so a failure names the stage that made it."""
    exL, exR = amd.ORBextractor(nf, 1.2, 8, ini, mn), amd.ORBextractor(nf, 1.2, 8, ini, mn)
    kL, dL = exL(L)
    kR, dR = exR(R)
    assert kL.tobytes() == ref[0].tobytes() and np.array_equal(dL, ref[1]), what + ": left extraction"
    assert kR.tobytes() == ref[2].tobytes() and np.array_equal(dR, ref[3]), what + ": right extraction"
    return exL, exR, len(kL)


def _assert_same_stereo(got, ref, what):
    for name, g, r in (("u_right", got[0], ref[0]), ("depth", got[1], ref[1])):
        assert g.shape == r.shape, f"{what}: {name} count"
        bad = np.nonzero(g.view(np.uint32) != r.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]} got {g[bad[:4]]} want {r[bad[:4]]}"


@pytest.mark.parametrize("name,kind", [("kitti04", "wide"), ("euroc", "wide"), ("d435i", "wide"), ("small", "wide"),
                                       ("kitti04", "dense"), ("euroc", "dense")])
def test_stereo_shipped_cameras(amd, oracle_mod, name, kind):
    """Each camera with its own image size (row table of H + 2 entries, sort LDS of 2 * (H + 2) +
    2 * cap words), feature count, FAST thresholds, bf and mb. "wide": disparities up to 1.15 fx, so
    `kx >= minU` and `disparity < maxD` both reject; "dense": synth.stereo_pair's 2..96 px."""
    cam = fc.CAMERAS[name]
    mb = fc.mb_of(cam.bf, cam.fx)
    if kind == "wide":
        L, R, *ref, ((u_ref, d_ref), _) = fc.wide_reference(oracle_mod, name)
    else:
        L, R = synth.stereo_pair(cam.h, cam.w, fc.WIDE_SEED)
        *ref, ((u_ref, d_ref),) = fc.stereo_reference(oracle_mod, L, R, cam.nf, cam.ini, cam.min, cam.bf, (mb,))
    assert (u_ref >= 0).sum() >= 50
    exL, exR, n = _drop_in(amd, L, R, cam.nf, cam.ini, cam.min, ref, f"{name} {kind}")
    _assert_same_stereo(amd.compute_stereo_matches(exL, exR, n, cam.bf, mb), (u_ref, d_ref), f"{name} {kind}")


def test_stereo_maxd_binds(amd, oracle_mod):
    """The "small" camera's wide pair matched with mb and with mb / 4 (maxD = fx and 4 fx): both
    bit-equal to the oracle, and different from each other in >= 20 entries -- the window test is
    live on the GPU, not only in the oracle."""
    cam = fc.CAMERAS["small"]
    mb = fc.mb_of(cam.bf, cam.fx)
    L, R, *ref, (ref1, ref4) = fc.wide_reference(oracle_mod, "small")
    exL, exR, n = _drop_in(amd, L, R, cam.nf, cam.ini, cam.min, ref, "small")
    got1 = amd.compute_stereo_matches(exL, exR, n, cam.bf, mb)
    got4 = amd.compute_stereo_matches(exL, exR, n, cam.bf, mb / 4)
    _assert_same_stereo(got1, ref1, "maxD = fx")
    _assert_same_stereo(got4, ref4, "maxD = 4 fx")
    assert (got1[0].view(np.uint32) != got4[0].view(np.uint32)).sum() >= 20


def test_stereo_zero_disparity(amd, oracle_mod):
    """Keypoints on a mirror axis match themselves with SAD(-1) == SAD(+1): disparity exactly 0, the
    `disparity <= 0` branch (Frame.cc:1092-1096). mvDepth = mbf / 0.01f at exactly the oracle's
    indices, mvuRight = float(double(uL) - 0.01) there."""
    L, R = fc.mirror_pair(240, 321, 5)
    *ref, ((u_ref, d_ref),) = fc.stereo_reference(oracle_mod, L, R, 500, 20, 7, KITTI_BF, (0.537,))
    exL, exR, n = _drop_in(amd, L, R, 500, 20, 7, ref, "mirror")
    u, d = amd.compute_stereo_matches(exL, exR, n, KITTI_BF, 0.537)
    _assert_same_stereo((u, d), (u_ref, d_ref), "mirror")
    far = np.flatnonzero(d_ref == fc.far_depth(KITTI_BF))
    assert far.size >= 3
    np.testing.assert_array_equal(np.flatnonzero(d == fc.far_depth(KITTI_BF)), far)
    np.testing.assert_array_equal(u[far], (ref[0]["x"][far].astype(np.float64) - 0.01).astype(np.float32))


def test_stereo_identical_pair(amd, oracle_mod):
    """R == L: every match has SAD 0, the median is 0 and the cut `dist < 2.1 * median` keeps none
    (Frame.cc:1112-1127): all -1, as the oracle."""
    L = synth.textured_image(240, 320, 23)
    *ref, ((u_ref, d_ref),) = fc.stereo_reference(oracle_mod, L, L, 500, 20, 7, KITTI_BF, (0.537,))
    assert (u_ref == -1).all() and (d_ref == -1).all() and len(u_ref) > 100
    exL, exR, n = _drop_in(amd, L, L, 500, 20, 7, ref, "identical")
    _assert_same_stereo(amd.compute_stereo_matches(exL, exR, n, KITTI_BF, 0.537), (u_ref, d_ref), "identical")


@pytest.mark.parametrize("name", ["euroc", "d435i"])
def test_stereo_pipeline_shipped_cameras(amd, oracle_mod, name):
    """StereoPipeline at a shipped camera's size, feature count, thresholds and bf / mb: 3 wide pairs
    over 2 engines (chunks of 2 and 1), keypoints, descriptors, mvuRight and mvDepth per pair."""
    import torch
    cam = fc.CAMERAS[name]
    mb = fc.mb_of(cam.bf, cam.fx)
    pairs = [fc.wide_reference(oracle_mod, name)[:2]] + [fc.camera_wide_pair(cam, s) for s in (33, 34)]
    dev = torch.from_numpy(np.stack([im for pr in pairs for im in pr])).cuda()
    pl = amd.StereoPipeline(cam.nf, iniThFAST=cam.ini, minThFAST=cam.min, n_engines=2)
    pl.reserve(cam.w, cam.h, 3)
    torch.cuda.synchronize()
    pl.stereo_batch(dev.data_ptr(), 3, cam.w, cam.h, cam.w, cam.h * cam.w, cam.bf, mb)
    torch.cuda.synchronize()
    for p, (L, R) in enumerate(pairs):
        if p == 0:
            kL, dL, kR, dR, ((u, d), _) = fc.wide_reference(oracle_mod, name)[2:]
        else:
            kL, dL, kR, dR, ((u, d),) = fc.stereo_reference(oracle_mod, L, R, cam.nf, cam.ini, cam.min, cam.bf, (mb,))
        _check_pair((*pl.fetch(p), *[a[:len(kL)] for a in pl.stereo_fetch(p)]), (kL, dL, kR, dR, u, d), f"{name} pair {p}")
    pl.close()


def _capacity(amd, ex):
    import ctypes
    cap = ctypes.c_int()
    assert amd.lib().orbx_capacity(ex.handle, ctypes.byref(cap)) == 0
    return cap.value


def test_stereo_capacity_limit(amd, oracle_mod):
    """The matcher's documented limit (include/orbslam2_amd.h, orbm_stereo_match): the right-keypoint
    sort keeps 2 * (H + 2) + 2 * capacity words in LDS and refuses more than 64 KB with ORBX_EINVAL
    (status -1). At 752 x 480 the capacity is nfeatures + 24 (N + 3 slots on each of 8 levels), so
    7686 features fill the 16384 words exactly and run, bit-equal to the oracle; 7687 and 16000
    (>= 131 KB) extract but do not match; the same two engines' successors at 1200 features then
    match the oracle."""
    cam = fc.CAMERAS["euroc"]
    mb = fc.mb_of(cam.bf, cam.fx)
    L, R = fc.wide_reference(oracle_mod, "euroc")[:2]
    for nf in (7687, 16000):
        exL, exR = amd.ORBextractor(nf), amd.ORBextractor(nf)
        kL, _ = exL(L)
        kR, _ = exR(R)
        assert len(kL) > 1200 and len(kR) > 1200
        assert 2 * (cam.h + 2) + 2 * _capacity(amd, exL) > 16384
        with pytest.raises(amd.OrbslamError, match="status -1"):
            amd.compute_stereo_matches(exL, exR, len(kL), cam.bf, mb)
        exL.close()
        exR.close()
    for nf in (1200, 7686):
        *ref, ((u_ref, d_ref),) = fc.stereo_reference(oracle_mod, L, R, nf, 20, 7, cam.bf, (mb,))
        exL, exR, n = _drop_in(amd, L, R, nf, 20, 7, ref, f"nf {nf}")
        if nf == 7686:
            assert 2 * (cam.h + 2) + 2 * _capacity(amd, exL) == 16384
        _assert_same_stereo(amd.compute_stereo_matches(exL, exR, n, cam.bf, mb), (u_ref, d_ref), f"nf {nf}")
