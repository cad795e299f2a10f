"""The matcher test inputs of matcher_cases.py reach what they are built to reach, shown with the CPU
oracle alone: node sizes beyond a wavefront, crowd members on the intended lanes of the resolve kernels'
64-query windows with the ownership known by construction, keypoints outside a grid with fractional
bounds, decisions taken exactly at a gate / at float equality / at a tie, rotation bins on their edges,
and the documented keypoint capacities. The GPU tests compare bits on the same inputs; the floors here
(half of the measured oracle counts, given next to each case) keep a later change to a generator from
turning a case vacuous. They are conditions on the inputs, not measurements."""
import hashlib

import numpy as np
import pytest

import matcher_cases as mc
from track_cases import crowd_expected_owner, crowd_problem, crowd_window_replay

F32 = np.float32


def _digest(o, h):
    if isinstance(o, dict):
        for k in sorted(o):
            if k != "crowd":
                h.update(k.encode())
                _digest(o[k], h)
    elif o is None:
        h.update(b"None")
    else:
        a = np.asarray(o)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())


def test_default_crowd_is_unchanged():
    """crowd_problem() gained arguments; its default arrays are the ones the earlier tests ran on."""
    h = hashlib.sha256()
    _digest(crowd_problem(), h)
    assert h.hexdigest() == "7b791d35bf8ae5d43ad5ee3d3905fc208d5d2398ac73ebdd44af6d60a9f4834c"


def _owners(own):
    return {int(k): int(own[k]) for k in np.nonzero(own >= 0)[0]}


# what crowd_window_replay() must report: (kernel form, stop) = a member that stops a window on that lane.
# want 2 = track_local_resolve_kernel, want 1 = track_frame_resolve_kernel (motion, relocalisation, Sim3)
CROWD_STOPS = {
    "straddle": [(2, (61, 61, "conflict")), (1, (61, 61, "conflict")), (2, (64, 0, "fallback")), (1, (64, 0, "fallback"))],
    "lane63": [(1, (130, 63, "fallback")), (1, (141, 10, "fallback")), (1, (151, 9, "fallback")),
               (1, (215, 63, "fallback")), (2, (130, 62, "fallback")), (2, (215, 63, "fallback"))],
    "lane63_local": [(2, (131, 63, "fallback")), (2, (142, 10, "fallback")), (2, (152, 9, "fallback")),
                     (2, (216, 63, "fallback")), (1, (216, 63, "fallback"))],
    "last_exhausted": [(2, (68, 0, "fallback")), (1, (68, 0, "fallback")), (1, (61, 61, "conflict"))],
    "two_crowds": [(2, (60, 60, "conflict")), (1, (60, 60, "conflict")), (1, (66, 0, "fallback")), (1, (67, 0, "fallback"))],
    "no_obs": [(2, (51, 51, "conflict")), (1, (51, 51, "conflict")), (1, (57, 0, "fallback"))],
}


@pytest.mark.parametrize("name", list(mc.CROWDS))
def test_crowd_ownership(oracle_mod, name):
    """Keypoint j of crowd c goes to the member crowd_expected_owner() names, in all four searches, and no
    ordinary point matches anything (so nothing but the crowd stops a window). crowd_window_replay(), the
    kernels' 64-query schedule restated, ends in the same ownership and puts the stops on the lanes of
    CROWD_STOPS. Measured local / frame / relocalisation / Sim3 matches: straddle 13 13 13 7, lane63 and
    lane63_local 8 8 8 7, last_exhausted 6 6 6 6, two_crowds 26 26 26 14, no_obs 25 25 13 7, n64 / n65 / n200
    13 13 13 7."""
    p = mc.track_case("crowd_" + name)
    mem = p["crowd"]["members"]
    flat = sorted(q for m_ in mem for q in m_)
    exp = crowd_expected_owner(p, 100)
    nm, own, _ = oracle_mod.search_local_points(p)
    assert _owners(own) == exp and nm >= len(exp) >= 6
    nm, own = oracle_mod.search_by_projection_frame(p, th=15.0, check_ori=False)
    assert _owners(own) == exp
    blocks = crowd_expected_owner(p, 100, True)
    nm, own = oracle_mod.search_by_projection_keyframe(p, th=10.0, orb_dist=100, check_ori=False)
    assert _owners(own) == blocks and nm == len(blocks)
    low = crowd_expected_owner(p, 50, True)
    nm, m = oracle_mod.search_by_projection_sim3(p, 10)
    assert _owners(m) == low and nm == len(low) >= 6
    stops = {}
    for want, gate, every in ((2, 100, False), (1, 100, False), (1, 100, True), (1, 50, True)):
        owner, st = crowd_window_replay(p, want, gate, every)
        assert owner == crowd_expected_owner(p, gate, every), (want, gate, every)
        if not every:
            stops[want] = st
    for want, stop in CROWD_STOPS.get(name, []):
        assert stop in stops[want], (want, stop)
    # more fallbacks than one window holds lanes is not needed; at least one of each kind everywhere
    assert all({k for _, _, k in stops[w]} == {"conflict", "fallback"} for w in (1, 2))
    if name == "lane63":          # two fallbacks inside one window: no stop between queries 131 and 151 but 141
        assert [s for s in stops[1] if 131 <= s[0] <= 151] == [(141, 10, "fallback"), (151, 9, "fallback")]
    if name == "last_exhausted":  # the last query is a member with every keypoint taken
        assert flat[-1] == len(p["map"]["Xw"]) - 1 and len(exp) == 6 < len(flat)
    if name == "no_obs":
        # member 2j - 1 (no observations) takes keypoint j without blocking it, member 2j takes it again: the frame
        # search pushes keypoints 1..12 into the rotation histogram twice, keypoint 0 once (25 entries), and
        # nmatches drops by one per removed entry
        assert int((p["map"]["flags"][flat] == 0).sum()) == 15
        kp, la = p["frame"]["keys_un"], float(p["last"]["keys_un"]["angle"][0])
        mult = np.array([1] + [2] * 12)
        bins = np.array([mc.rot_bin(la, float(kp["angle"][j])) for j in range(13)])
        keep = mc.three_maxima(np.bincount(bins, weights=mult, minlength=30).astype(int))
        survive = int(mult[np.isin(bins, list(keep))].sum())
        once = mc.three_maxima(np.bincount(bins, minlength=30))
        nm, own = oracle_mod.search_by_projection_frame(p, th=15.0, check_ori=True)
        assert nm == survive == 8 and int((own >= 0).sum()) == int(np.isin(bins, list(keep)).sum()) < survive
        print("kept bins with / without the double entries:", sorted(keep), sorted(once))


# measured BoW / triangulation / stereo-only triangulation / BoW-KF: mod3 108 59 14 34, one 154 74 24 44,
# skewed 117 57 12 37, sizes 123 63 14 37, one4096 907 441 102 247
BOW_FLOORS = {"mod3": (54, 29, 7, 17), "one": (77, 37, 12, 22), "skewed": (58, 28, 6, 18), "sizes": (61, 31, 7, 18),
              "one4096": (453, 220, 51, 123)}


@pytest.mark.parametrize("name", list(BOW_FLOORS))
def test_skewed_feature_vectors(oracle_mod, name):
    """The largest B-node: 202 (node % 3), 600 / 4096 (one node), 370 (nodes < 60 merged), 128 (exact sizes)."""
    p = mc.bow_case(name)
    sb = mc.node_sizes(p["B"])
    largest = {"mod3": 202, "one": 600, "skewed": 370, "sizes": 128, "one4096": 4096}[name]
    assert max(sb.values()) == largest > 64
    got = (oracle_mod.search_by_bow(p)[0], len(oracle_mod.search_for_triangulation(p)),
           len(oracle_mod.search_for_triangulation(p, True)), oracle_mod.search_by_bow_kf(p)[0])
    print(name, got)
    assert all(g >= f for g, f in zip(got, BOW_FLOORS[name]))
    if name == "one4096":
        assert len(p["A"]["keys_un"]) == len(p["B"]["keys_un"]) == 4096


def test_node_sizes_case(oracle_mod):
    p = mc.bow_case("sizes")
    sa, sb = mc.node_sizes(p["A"]), mc.node_sizes(p["B"])
    assert [sb[i] for i in range(4)] == [63, 64, 65, 128] and all(sa[i] > 20 for i in range(4))
    assert mc.SPILL in sb and mc.SPILL not in sa and mc.ONLY_A in sa and mc.ONLY_A not in sb
    na = mc.feature_nodes(p["A"])
    for node in (mc.NO_MP, mc.ALL_BAD):
        assert sa[node] >= 3 and sb[node] >= 3
    dead = np.nonzero((na == mc.NO_MP) | (na == mc.ALL_BAD) | (na == mc.ONLY_A))[0]
    _, m12 = oracle_mod.search_by_bow_kf(p)
    assert (m12[dead] == -1).all()
    tri = oracle_mod.search_for_triangulation(p)
    assert not (set(tri[:, 0].tolist()) & set(np.nonzero((na == mc.ALL_BAD) | (na == mc.ONLY_A))[0].tolist()))
    # matches inside the four sized nodes, so their strides do work
    nb = mc.feature_nodes(p["B"])
    _, m = oracle_mod.search_by_bow(p)
    assert all(int(((m >= 0) & (nb == g)).sum()) >= 3 for g in range(4))


# measured: keypoints outside the grid, then local / frame / reloc (reloc problem) / Sim3 projection / fuse <= 50 /
# fuse-Sim3 <= 50 / SearchBySim3: tum640 80 340 90 85 322 324 348 138, neg640 7 375 105 100 354 356 384 158,
# w752 22 369 119 102 348 348 383 163, hd720 7 395 106 113 369 375 392 166
BOUNDS_FLOORS = {"tum640": (40, 170, 45, 42, 161, 162, 174, 69), "neg640": (3, 187, 52, 50, 177, 178, 192, 79),
                 "w752": (11, 184, 59, 51, 174, 174, 191, 81), "hd720": (3, 197, 53, 56, 184, 187, 196, 83)}


@pytest.mark.parametrize("name", list(mc.CAMERAS))
def test_bounds_cases(oracle_mod, name):
    p = mc.bounds_case(oracle_mod, name)
    b = mc.camera_bounds(oracle_mod, name)
    if name == "tum640":
        assert [round(v, 3) for v in b] == [10.801, 626.048, 14.669, 473.312]
    fr = p["frame"]
    assert (fr["min_x"], fr["max_x"], fr["min_y"], fr["max_y"]) == b == tuple(p["last"][k] for k in
                                                                                ("min_x", "max_x", "min_y", "max_y"))
    kp = fr["keys_un"]
    px, py, inside = mc.pos_in_grid(kp["x"], kp["y"], b)
    e0 = len(kp) - mc.N_EDGE_KP
    # keypoints exactly on the bounds: min is cell 0, max is one past the last cell
    assert (px[e0], px[e0 + 1]) == (0, mc.GRID_COLS) and inside[e0] and not inside[e0 + 1]
    for j in range(3, 15, 2):      # the pairs around a cell boundary land in neighbouring cells
        assert px[e0 + j + 1] == px[e0 + j] + 1
    assert int((kp["x"] == np.rint(kp["x"])).sum()) >= len(kp) // 5 - mc.N_EDGE_KP   # integer pixel coordinates
    nm, own, view = oracle_mod.search_local_points(p)
    got = (int((~inside).sum()), nm, oracle_mod.search_by_projection_frame(p)[0],
           oracle_mod.search_by_projection_keyframe(mc.bounds_case(oracle_mod, name, "reloc"))[0],
           oracle_mod.search_by_projection_sim3(p, 10)[0], int((oracle_mod.fuse_candidates(p, 3.0)[1] <= 50).sum()),
           int((oracle_mod.fuse_sim3_candidates(p, 4.0)[1] <= 50).sum()),
           oracle_mod.search_by_sim3(mc.bounds_case(oracle_mod, name, "pair"), 7.5)[0])
    print(name, b, got)
    assert all(g >= f for g, f in zip(got, BOUNDS_FLOORS[name]))
    # map points projecting exactly onto a bound: the Frame gate keeps u == min_x and u == max_x, the KeyFrame
    # gate (int bounds, u >= min && u < max) keeps (int)min_x and drops max_x, (int)max_x and a fractional min_x
    fuse_idx, _ = oracle_mod.fuse_candidates(p, 3.0)
    ex = p["exact"]
    assert float(F32(b[1])) in ex and float(int(b[1])) in ex
    if name != "tum640":
        assert float(F32(b[0])) in ex and float(int(b[0])) in ex
    for u, (i, k) in ex.items():
        in_frame = F32(b[0]) <= F32(u) <= F32(b[1])
        assert view["in_view"][i] == int(in_frame)
        if in_frame:
            assert view["proj_x"][i] == F32(u)
        in_kf = int(b[0]) <= u < int(b[1])
        assert (fuse_idx[i] >= 0) == (in_kf and u < b[0] + 1), (u, fuse_idx[i])
        if u < b[0] + 1 and in_frame:
            assert own[k] == i
    assert not view["in_view"][list(p["z_points"])].any()


def _frame_levels(p, L):
    """The level range SearchByProjection(CurrentFrame, LastFrame) uses (ORBmatcher.cc:1757-1771, 1830-1838)."""
    T = np.asarray(p["frame"]["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    Tl = np.asarray(p["last"]["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    tlc = Tl[:, :3] @ (-T[:, :3].T @ T[:, 3]) + Tl[:, 3]
    if tlc[2] > p["frame"]["mb"]:
        return 0, 99
    if -tlc[2] > p["frame"]["mb"]:
        return -99, 0
    return -1, 1


def _spot_owner(p, own, i):
    """keypoint taken by map point i (or -1) from a keypoint -> map point array"""
    k = [k for k in p["spots"][i]["kp"] if own[k] == i]
    assert len(k) <= 1
    return k[0] if k else -1


def test_gates(oracle_mod):
    """The candidate at distance g is taken iff g <= gate: TH_HIGH 100 (local, frame, SearchBySim3), ORBdist (64 and
    100, relocalisation), TH_LOW 50 (Sim3 projection); Fuse reports g itself (256 / INT_MAX never appear)."""
    p = mc.track_case("gates")
    D = mc.GATE_DISTS
    own = oracle_mod.search_local_points(p)[1]
    assert [_spot_owner(p, own, i) >= 0 for i in range(len(D))] == [g <= 100 for g in D]
    own = oracle_mod.search_by_projection_frame(p, check_ori=False)[1]
    assert [_spot_owner(p, own, i) >= 0 for i in range(len(D))] == [g <= 100 for g in D]
    for od in (64, 100):
        own = oracle_mod.search_by_projection_keyframe(p, orb_dist=od, check_ori=False)[1]
        assert [_spot_owner(p, own, i) >= 0 for i in range(len(D))] == [g <= od for g in D]
    m = oracle_mod.search_by_projection_sim3(p, 10)[1]
    assert [_spot_owner(p, m, i) >= 0 for i in range(len(D))] == [g <= 50 for g in D]
    for bi, bd in (oracle_mod.fuse_candidates(p, 3.0), oracle_mod.fuse_sim3_candidates(p, 4.0)):
        assert bd.tolist() == list(D) and bi.tolist() == [s["kp"][0] for s in p["spots"]]
    nf, m12 = oracle_mod.search_by_sim3(mc.as_pair(p), 7.5)
    assert [m12[s["kp"][0]] == i for i, s in enumerate(p["spots"])] == [g <= 100 for g in D] and nf == 8


@pytest.mark.parametrize("nnratio", [r for r, _, _ in mc.RATIOS])
def test_ratio_at_float_equality(oracle_mod, nnratio):
    """Spot 2k (same level) is rejected iff float32(d1) > float32(nnratio) * float32(d2); spot 2k + 1 (different
    levels) is always taken. 0.75 * 100 == 75 and 0.6f * 100 rounds to 60: kept; 0.8f * 100 and 0.9f * 100 round
    to 80 and 90: kept too -- while the neighbouring ratios reject, so each run holds both outcomes."""
    p = mc.track_case("ratio")
    own = oracle_mod.search_local_points(p, nnratio=nnratio)[1]
    seen = set()
    for k, (_, d1, d2) in enumerate(mc.RATIOS):
        rejected = bool(F32(d1) > F32(nnratio) * F32(d2))
        seen.add(rejected)
        assert (_spot_owner(p, own, 2 * k) < 0) == rejected, (nnratio, d1, d2)
        assert _spot_owner(p, own, 2 * k) == mc.local_decision(p, 2 * k, nnratio)
        assert _spot_owner(p, own, 2 * k + 1) == p["spots"][2 * k + 1]["kp"][0]
    assert seen == {True, False} or nnratio == 0.9


def test_ties(oracle_mod):
    """Equal minimum distances: the first in candidate order wins in the frame, relocalisation, Sim3 and both Fuse
    searches; the local search takes the first when the tied two are on different levels and rejects the
    point when they share one (bestDist > nnratio * bestDist2)."""
    p = mc.track_case("ties")
    n = len(p["spots"])
    own = oracle_mod.search_local_points(p)[1]
    dec = [mc.local_decision(p, i, 0.8) for i in range(n)]
    assert [_spot_owner(p, own, i) for i in range(n)] == dec
    assert [d >= 0 for d in dec] == [False, True, False] * 2
    lo, hi = _frame_levels(p, 1)
    own = oracle_mod.search_by_projection_frame(p, check_ori=False)[1]
    assert [_spot_owner(p, own, i) for i in range(n)] == [mc.first_min_decision(p, i, 100, lo, hi)[0] for i in range(n)]
    own = oracle_mod.search_by_projection_keyframe(p, check_ori=False)[1]
    assert [_spot_owner(p, own, i) for i in range(n)] == [mc.first_min_decision(p, i, 100, -1, 1)[0] for i in range(n)]
    first = [mc.first_min_decision(p, i, 50, -1, 0)[0] for i in range(n)]
    assert min(first) >= 0
    # the winner is not simply the lowest keypoint index everywhere
    assert any(f != p["spots"][i]["kp"][0] for i, f in enumerate(first))
    m = oracle_mod.search_by_projection_sim3(p, 10)[1]
    assert [_spot_owner(p, m, i) for i in range(n)] == first
    assert oracle_mod.fuse_candidates(p, 3.0)[0].tolist() == first
    assert oracle_mod.fuse_sim3_candidates(p, 4.0)[0].tolist() == first


@pytest.mark.parametrize("name", mc.ROT_NAMES)
def test_rotation_histogram(oracle_mod, name):
    """The matches that survive the rotation check are those whose bin -- floor(float32(rot * 30 / 360.0f) + 0.5),
    30 -> 0 -- is among ComputeThreeMaxima's kept bins, for the frame, relocalisation and both SearchByBoW
    searches. edges: bins 0, 1, 2 hold 8 + their edge cases; tie_max: four bins of 5, the first three stay;
    ten_percent: 20, 2, 1 keeps two bins; below: 30, 2, 2 keeps one; one_bin."""
    pairs = mc.ROT_SETS[name]
    keep, bins = mc.rot_survivors(pairs)
    counts = np.bincount(bins, minlength=30)
    if name == "edges":
        assert mc.rot_bin(56.0, 50.0) == 1 and mc.rot_bin(6.0, 0.0) == 1 and mc.rot_bin(18.0, 0.0) == 2
        assert mc.rot_bin(354.0, 0.0) == 0 and mc.rot_bin(360.0, 0.0) == 0 and mc.rot_bin(10.0, 20.0) == 29
        assert mc.rot_bin(5.999, 0.0) == 0 and mc.rot_bin(0.0, 6.0) == 0 and mc.rot_bin(0.0, 18.0) == 29
        assert not all(keep) and sum(keep) > 30
    if name == "tie_max":
        assert sorted(counts[counts > 0].tolist()) == [5, 5, 5, 5] and sum(keep) == 15
    if name == "ten_percent":
        assert sorted(counts[counts > 0].tolist()) == [1, 2, 20] and sum(keep) == 22
    if name == "below":
        assert sorted(counts[counts > 0].tolist()) == [2, 2, 30] and sum(keep) == 30
    if name == "one_bin":
        assert all(keep) and len(keep) == 12
    p = mc.track_case("rot_" + name)
    for nm, own in (oracle_mod.search_by_projection_frame(p), oracle_mod.search_by_projection_keyframe(p)):
        assert [_spot_owner(p, own, i) >= 0 for i in range(len(pairs))] == keep and nm == sum(keep)
    q = mc.bow_case("rot_" + name)
    nm, m = oracle_mod.search_by_bow(q)
    assert (m >= 0).tolist() == keep and nm == sum(keep)
    nm, m12 = oracle_mod.search_by_bow_kf(q)
    assert (m12 >= 0).tolist() == keep and nm == sum(keep)


def test_predict_scale_and_viewing_cos(oracle_mod):
    """Spots 0..7: max_dist / dist == 1.2f^k in float32 and the level is ceil(logf(ratio) / logf(1.2f)) on the
    float32 quotient; 8 / 9 clamp to level 0 / 7. Spots 10..14: viewCos is exactly 0.5f (in view), the two
    float32 around 0.998 (radius 4.0 below, 2.5 above: the keypoint 3.5 px away at level 1 is inside only below),
    just above 0.5f and 1.0f."""
    p = mc.track_case("scale")
    nm, own, view = oracle_mod.search_local_points(p)
    Ow = np.asarray(p["frame"]["Ow"], F32)
    ls = F32(p["frame"]["log_scale_factor"])
    for k in range(8):
        PO = (p["map"]["Xw"][k] - Ow).astype(np.float64)
        ratio = p["map"]["max_dist"][k] / F32(np.sqrt((PO * PO).sum()))
        assert ratio == p["frame"]["scale_factors"][k] == F32(p["spots"][k]["ratio"])
        lvl = int(np.ceil(F32(F32(oracle_mod.logf(float(ratio))) / ls)))
        assert view["level"][k] == min(max(lvl, 0), 7)
        assert abs(int(view["level"][k]) - k) <= 1
    print("levels at 1.2f^k:", view["level"][:8].tolist())
    assert view["level"][8] == 0 and view["level"][9] == 7 and view["in_view"][:15].all()
    cos = [p["spots"][i]["view_cos"] for i in range(10, 15)]
    assert view["view_cos"][10:15].tolist() == cos
    assert cos[0] == 0.5 and cos[1] < 0.998 < cos[2] and np.nextafter(F32(cos[1]), F32(1)) == F32(cos[2])
    wide = [_spot_owner(p, own, i) >= 0 for i in range(10, 15)]
    assert wide == [True, True, False, True, False]


@pytest.mark.parametrize("nnratio", [0.6, 0.7, 0.75, 0.8, 0.9])
def test_bow_equality(oracle_mod, nnratio):
    """Every A-feature of bow_equality_problem decides as the sequential rule says (bow_decisions), for SearchByBoW
    (KF, F) (<= TH_LOW) and (KF, KF) (< TH_LOW); the intended outcomes hold: 50 passes only the former, ties for
    the best are rejected in different lanes, in one lane and three ways, and the second query of the last
    cell finds position 70 taken and moves to 100."""
    p = mc.bow_case("equality")
    A, B = p["A"], p["B"]
    exp = mc.bow_decisions(p, nnratio, False)
    nm, m = oracle_mod.search_by_bow(p, nnratio, False)
    got = np.full(len(A["keys_un"]), -1, np.int64)
    for ib in np.nonzero(m >= 0)[0]:
        got[m[ib]] = ib                      # A["mp"] = arange: the map point is the A index
    assert got.tolist() == exp.tolist() and nm == int((exp >= 0).sum())
    exps = mc.bow_decisions(p, nnratio, True)
    nm, m12 = oracle_mod.search_by_bow_kf(p, nnratio, False)
    assert m12.tolist() == exps.tolist() and nm == int((exps >= 0).sum())   # B["mp"] = arange
    cells = p["cells"]
    assert (exp[0] >= 0, exp[1] >= 0, exp[2] >= 0) == (True, True, False)
    assert (exps[0] >= 0, exps[1] >= 0, exps[2] >= 0) == (True, False, False)
    for k, (r, d1, d2) in enumerate(mc.BOW_RATIOS):
        ia = cells[3 + k]["a"][0]
        assert (exp[ia] >= 0) == bool(d1 <= 50 and F32(d1) < F32(nnratio) * F32(d2))
    t = 3 + len(mc.BOW_RATIOS)
    assert [int(exp[cells[t + j]["a"][0]]) for j in range(3)] == [-1, -1, -1]
    c = cells[t + 3]
    assert exp[c["a"][0]] == c["b0"] + 100
    c = cells[t + 4]
    assert exp[c["a"]].tolist() == [c["b0"] + 70, c["b0"] + 100]


@pytest.mark.parametrize("stride", [1, 64])
def test_bow_ties_in_a_node(oracle_mod, stride):
    """An identical second candidate `stride` positions later in the one 600-feature node: both SearchByBoW forms
    drop the match (best == second fails the ratio test), SearchForTriangulation moves it to the later one."""
    p, pairs = mc.bow_tie_problem(oracle_mod, "tri", stride)
    assert len(pairs) == 8
    tri = {int(a): int(b) for a, b in oracle_mod.search_for_triangulation(p)}
    assert all(tri.get(ia) == ib + stride for ia, ib in pairs)
    p, pairs = mc.bow_tie_problem(oracle_mod, "bow", stride)
    assert len(pairs) == 8
    _, m = oracle_mod.search_by_bow(p)
    for ia, ib in pairs:
        assert p["A"]["mp"][ia] not in (m[ib], m[ib + stride])
    p, pairs = mc.bow_tie_problem(oracle_mod, "bowkf", stride)
    assert len(pairs) == 8
    _, m12 = oracle_mod.search_by_bow_kf(p)
    assert all(m12[ia] != p["B"]["mp"][ib] for ia, ib in pairs)


# measured local / frame / reloc / Sim3 projection / fuse <= 50 / fuse-Sim3 <= 50:
# quant1 385 123 122 573 436 514, quant2 385 122 124 578 436 514, quant4 387 127 125 575 436 514;
# BoW / triangulation / BoW-KF: quant1 31 78 26, quant2 75 81 28, quant4 97 89 43
@pytest.mark.parametrize("name", ["quant1", "quant2", "quant4"])
def test_quantised_problems_stay_non_trivial(oracle_mod, name):
    p = mc.track_case(name)
    got = (oracle_mod.search_local_points(p)[0], oracle_mod.search_by_projection_frame(p)[0],
           oracle_mod.search_by_projection_keyframe(p)[0], oracle_mod.search_by_projection_sim3(p, 10)[0],
           int((oracle_mod.fuse_candidates(p, 3.0)[1] <= 50).sum()),
           int((oracle_mod.fuse_sim3_candidates(p, 4.0)[1] <= 50).sum()))
    print(name, got)
    assert all(g >= f for g, f in zip(got, (192, 61, 61, 286, 218, 257)))
    nb = int(name[-1])
    assert not p["frame"]["desc"][:, nb:].any() and not p["map"]["desc"][:, nb:].any()
    q = mc.bow_case(name)
    got = (oracle_mod.search_by_bow(q)[0], len(oracle_mod.search_for_triangulation(q)), oracle_mod.search_by_bow_kf(q)[0])
    print(name, got)
    assert all(g >= f for g, f in zip(got, {"quant1": (15, 39, 13), "quant2": (37, 40, 14), "quant4": (48, 44, 21)}[name]))


# measured local / frame / reloc / Sim3 / fuse <= 50: cap8192 2964 1548 1840 2905 2855, cap8191 1012 686 816 993 992,
# cap4097 950 651 797 935 929, one_cell 150 51 47 271 75
CAP_FLOORS = {"cap8192": (1482, 774, 920, 1452, 1427), "cap8191": (506, 343, 408, 496, 496),
              "cap4097": (475, 325, 398, 467, 464), "one_cell": (75, 25, 23, 135, 37)}


@pytest.mark.parametrize("name", ["cap8192", "cap8191", "cap4097", "one_cell", "cap1"])
def test_capacity_cases(oracle_mod, name):
    p = mc.track_case(name)
    n = {"cap8192": 8192, "cap8191": 8191, "cap4097": 4097, "one_cell": 8192, "cap1": 1}[name]
    assert len(p["frame"]["keys_un"]) == n
    if name.startswith("cap"):
        assert len(p["last"]["keys_un"]) == n
    if name == "cap1":
        assert oracle_mod.search_local_points(p)[0] == 0
        return
    if name == "one_cell":
        fr = p["frame"]
        px, py, inside = mc.pos_in_grid(fr["keys_un"]["x"], fr["keys_un"]["y"],
                                        (fr["min_x"], fr["max_x"], fr["min_y"], fr["max_y"]))
        assert inside.all() and len(set(zip(px.tolist(), py.tolist()))) == 1
    got = (oracle_mod.search_local_points(p)[0], oracle_mod.search_by_projection_frame(p)[0],
           oracle_mod.search_by_projection_keyframe(p)[0], oracle_mod.search_by_projection_sim3(p, 10)[0],
           int((oracle_mod.fuse_candidates(p, 3.0)[1] <= 50).sum()))
    print(name, got)
    assert all(g >= f for g, f in zip(got, CAP_FLOORS[name]))


def test_search_by_sim3_pairs(oracle_mod):
    """SearchBySim3 inputs: the gates pair matches exactly the 8 spots at distance <= TH_HIGH; measured matches of
    the quantised pair 100 and of the 8192-keypoint pair 1326."""
    assert oracle_mod.search_by_sim3(mc.pair_case("gates"), 7.5)[0] == 8
    assert oracle_mod.search_by_sim3(mc.pair_case("quant2"), 7.5)[0] >= 50
    p = mc.pair_case("cap8192")
    assert len(p["kf1"]["keys_un"]) == len(p["kf2"]["keys_un"]) == 8192
    assert oracle_mod.search_by_sim3(p, 7.5)[0] >= 663


@pytest.mark.parametrize("name", mc.ROT_NAMES)
def test_triangulation_gate_and_histogram(oracle_mod, name):
    """SearchForTriangulation on real pairs of the one-node case: B-descriptors exactly 50 and 49 bits away are
    matched (`dist > TH_LOW` is the reject), 51 is not, and with the rotation check exactly the pairs whose bin
    ComputeThreeMaxima keeps remain. Pairs without / with the check: edges 45 37, tie_max 20 15, ten_percent
    23 22, below 34 30, one_bin 12 12."""
    p, used, dists = mc.tri_case(oracle_mod, name)
    rot = mc.ROT_SETS[name]
    assert dists[:len(rot)].count(50) >= 6 and dists[:len(rot)].count(49) >= 6 and dists[len(rot):] == [51] * 8
    for (ia, ib), d in zip(used, dists):
        assert mc.hamming(p["A"]["desc"][ia], p["B"]["desc"][ib]) == d
    plain = {tuple(r) for r in oracle_mod.search_for_triangulation(p, False, False).tolist()}
    assert plain == set(used[:len(rot)])
    keep, _ = mc.rot_survivors(rot)
    checked = {tuple(r) for r in oracle_mod.search_for_triangulation(p, False, True).tolist()}
    assert checked == {u for u, k in zip(used, keep) if k}
    assert len(oracle_mod.search_for_triangulation(p, True, True)) >= 6       # stereo-only: 12 8 8 11 6
