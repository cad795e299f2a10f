"""Hand-built projection / BoW matcher problems shared by the CPU and GPU tests.

Each builder returns the dict shapes oracle.* and amd.Tracker / amd.BowMatcher accept (extra keys
carry what the CPU test pins). The docstrings say which kernel path a case targets and why it
reaches it; tests/test_matcher_cases_cpu.py shows on the oracle alone that it does."""
import functools

import numpy as np

from orbslam2_amd import synth
from test_matcher_gpu import D_TUM, K_TUM
from track_cases import crowd_problem

GRID_COLS, GRID_ROWS, HISTO_LENGTH = 64, 48, 30
F32 = np.float32


# ---------------------------------------------------------------------------------------------
# a. skewed FeatureVectors (orb_bowmatch.hip bm_node_kernel: stride loop p = lane, lane + 64, ...;
#    claimed[p] for p >= 64; best / second from one lane)
# ---------------------------------------------------------------------------------------------
def feature_nodes(K: dict) -> np.ndarray:
    """Per-feature node id of a keyframe's FeatureVector (-1 = in no node)."""
    nodes = np.full(len(K["keys_un"]), -1, np.int64)
    for j, nd in enumerate(K["fv_nodes"]):
        nodes[K["fv_features"][K["fv_start"][j]:K["fv_start"][j + 1]]] = int(nd)
    return nodes


def with_nodes(K: dict, nodes: np.ndarray) -> dict:
    fvn, fvs, fvf = synth._fv_from_nodes(np.asarray(nodes, np.int64))
    return dict(K, fv_nodes=fvn, fv_start=fvs, fv_features=fvf)


def node_sizes(K: dict) -> dict:
    return {int(n): int(K["fv_start"][j + 1] - K["fv_start"][j]) for j, n in enumerate(K["fv_nodes"])}


NODE_MAPS = {"mod3": lambda n: n % 3, "one": lambda n: n * 0, "skewed": lambda n: np.where(n < 60, 0, n)}


def regroup(p: dict, name: str) -> dict:
    """bow_match_problem with every feature's node sent through NODE_MAPS[name] on both sides: nodes
    of hundreds to thousands of features, so a query's scan takes several 64-wide strides, claims land
    at positions >= 64 and one lane holds the best and the second-best candidate."""
    f = NODE_MAPS[name]
    return dict(p, A=with_nodes(p["A"], f(feature_nodes(p["A"]))), B=with_nodes(p["B"], f(feature_nodes(p["B"]))))


SPILL, ONLY_A, NO_MP, ALL_BAD = 900, 109, 108, 107


def node_sizes_problem(seed: int = 21, n: int = 700) -> dict:
    """B-nodes of exactly 63, 64, 65 and 128 features (nodes 0..3: the last stride of the scan is empty,
    full, one lane, and exactly two strides); node SPILL only in B, node ONLY_A only in A (the host's merge
    of the two node lists must skip both); node NO_MP whose A-features all lack a map point and node
    ALL_BAD whose A-features all hold a bad one (filtered by SearchByBoW; by SearchForTriangulation
    because they hold one): a shared node that does no work."""
    p = synth.bow_match_problem(seed, n=n, n_points=int(0.8 * n))
    na, nb = feature_nodes(p["A"]), feature_nodes(p["B"])
    ma, mb = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    targets, g, orig = [63, 64, 65, 128], 0, 0
    while g < len(targets):
        mb[nb == orig] = g
        ma[na == orig] = g
        orig += 1
        idx = np.nonzero(mb == g)[0]
        if len(idx) >= targets[g]:
            mb[idx[targets[g]:]] = SPILL
            g += 1
    assert orig < 97
    ma[ma < 0] = 10 + na[ma < 0]
    mb[mb < 0] = 10 + nb[mb < 0]
    mb[mb == ONLY_A] = SPILL
    A = dict(p["A"], mp=p["A"]["mp"].copy(), mp_bad=p["A"]["mp_bad"].copy())
    A["mp"][ma == NO_MP] = -1
    A["mp"][ma == ALL_BAD] = 0
    A["mp_bad"][ma == NO_MP] = 0
    A["mp_bad"][ma == ALL_BAD] = 1
    return dict(p, A=with_nodes(A, ma), B=with_nodes(p["B"], mb))


def duplicate_b(p: dict, pairs, stride: int) -> dict:
    """Ties in one node: for each (ia, ib) copy B's feature ib onto feature ib + stride of the same node (made
    for the one-node regrouping, where position in the node = feature index): the A-feature ia then has two
    candidates at the same distance. stride = 64 puts both in the same lane. BoW: the ratio test rejects
    (best == second). Triangulation: the later position wins (ORBmatcher.cc:990-1000 keeps no second best and
    its distance pre-check `dist > bestDist` lets an equal distance replace the best)."""
    B = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p["B"].items()}
    for _, ib in pairs:
        for k in ("keys_un", "desc", "u_right", "mp", "mp_bad"):
            B[k][ib + stride] = B[k][ib]
    return dict(p, B=B)


def quantise_bow(p: dict, nbytes: int) -> dict:
    """Descriptors zeroed beyond the first nbytes bytes on both sides: distances take 8 * nbytes + 1 values, so
    nearly every node scan holds ties for the best and the second-best candidate."""
    def q(K):
        d = K["desc"].copy()
        d[:, nbytes:] = 0
        return dict(K, desc=d)
    return dict(p, A=q(p["A"]), B=q(p["B"]))


def quantise_track(p: dict, nbytes: int) -> dict:
    """The same for a tracking problem (keypoint and map point descriptors): ties inside every window, for the
    dist << 16 | position keys of the kept top-4 lists and the first-minimum rule of the Fuse searches."""
    d = p["frame"]["desc"].copy()
    d[:, nbytes:] = 0
    md = p["map"]["desc"].copy()
    md[:, nbytes:] = 0
    return dict(p, frame=dict(p["frame"], desc=d), map=dict(p["map"], desc=md))


# ---------------------------------------------------------------------------------------------
# b. crowds across the resolve kernels' 64-query windows (orb_track.hip track_*_resolve_kernel)
# ---------------------------------------------------------------------------------------------
CROWDS = {
    # first claim on lane 60 of window 0; members 61.. conflict one by one, the fallbacks start at query 64
    "straddle": dict(n_kp_near=13, n_mp=20, lead=60, tail=10),
    # members 0..3 use up every later member's kept top-4. track_frame_resolve_kernel (takes one candidate):
    # window bases 0, 1, 2, 3, 67, so member 130 is a fallback on lane 63 with no stop before it; 141 and 151
    # are two fallbacks in the window based at 131; 215 = 152 + 63 is again lane 63 and the very last query.
    # track_local_resolve_kernel (takes best and second): member 3 is itself a fallback, the bases run 0, 1, 2,
    # 3, 4, 68, member 130 sits on lane 62 and only 215 on lane 63 -- "lane63_local" shifts the late members by
    # one so that 131 and 216 are on lane 63 there. crowd_window_replay() gives the lanes; the CPU test pins them
    "lane63": dict(n_kp_near=13, members=[[0, 1, 2, 3, 130, 141, 151, 215]]),
    "lane63_local": dict(n_kp_near=13, members=[[0, 1, 2, 3, 131, 142, 152, 216]]),
    # 6 keypoints, 9 members: members 66..68 are exhausted (rescan finds nothing), 68 is the last query
    "last_exhausted": dict(n_kp_near=6, n_mp=9, lead=60),
    # two crowds at different image places, alternating in query order from lane 58 on
    "two_crowds": dict(n_kp_near=13, members=[list(range(58, 98, 2)), list(range(59, 99, 2))], tail=5),
    # every second member has no observations: it takes a keypoint without blocking it, the next overwrites
    "no_obs": dict(n_kp_near=13, n_mp=30, lead=50, tail=3, no_obs_every=2),
    # the original construction at the sizes where the query count crosses one and three windows
    "n64": dict(n_kp_near=13, n_mp=64), "n65": dict(n_kp_near=13, n_mp=65), "n200": dict(n_kp_near=13, n_mp=200),
}


def sim3_stage(p: dict, scale: float = 1.0, matched=None) -> dict:
    """A tracking problem as the loop-closing searches take it: Scw = scale * [Rcw | tcw], vpMatched empty."""
    T = np.asarray(p["frame"]["Tcw"], np.float32).reshape(-1)[:12].reshape(3, 4)
    Scw = np.eye(4, dtype=np.float32)
    Scw[:3, :4] = (np.float32(scale) * T).astype(np.float32)
    if matched is None:
        matched = np.full(len(p["frame"]["keys_un"]), -1, np.int32)
    return dict(p, Scw=Scw, matched=matched)


def crowd(name: str) -> dict:
    return sim3_stage(crowd_problem(**CROWDS[name]))


# ---------------------------------------------------------------------------------------------
# c. image bounds, grid and cameras
# ---------------------------------------------------------------------------------------------
CAMERAS = {"tum640": (640, 480, "tum"), "neg640": (640, 480, "neg"), "w752": (752, 480, "plain"),
           "hd720": (1280, 720, "neg")}


def camera_bounds(oracle_mod, name: str):
    W, H, kind = CAMERAS[name]
    if kind == "tum":
        return tuple(float(b) for b in oracle_mod.image_bounds(W, H, K_TUM, D_TUM))
    if kind == "neg":
        return (-27.25, W + 27.5, -19.75, H + 19.5)
    return (0.0, float(W), 0.0, float(H))


def _with_bounds(fr: dict, b) -> dict:
    return dict(fr, min_x=float(b[0]), max_x=float(b[1]), min_y=float(b[2]), max_y=float(b[3]))


def pos_in_grid(x, y, b):
    """Frame::PosInGrid (Frame.cc:682-698) in float32; returns (px, py, inside)."""
    b = [F32(v) for v in b]
    iw, ih = F32(GRID_COLS) / (b[1] - b[0]), F32(GRID_ROWS) / (b[3] - b[2])
    fx, fy = (np.asarray(x, F32) - b[0]) * iw, (np.asarray(y, F32) - b[2]) * ih
    px = (np.sign(fx) * np.floor(np.abs(fx.astype(np.float64)) + 0.5)).astype(np.int64)   # roundf
    py = (np.sign(fy) * np.floor(np.abs(fy.astype(np.float64)) + 0.5)).astype(np.int64)
    return px, py, (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)


def _cell_edge_x(b, k):
    """The two neighbouring float32 x around (x - min_x) * inv_w == k + 0.5: the largest with a product below
    and the smallest with a product at or above (roundf sends the latter to cell k + 1)."""
    b0, iw = F32(b[0]), F32(GRID_COLS) / (F32(b[1]) - F32(b[0]))
    x = F32(b0 + F32(k + 0.5) / iw)
    cand = (np.array([x], F32).view(np.int32) + np.arange(-64, 65, dtype=np.int32)).view(F32)
    cand = np.sort(cand)
    prod = (cand - b0) * iw
    hi = int(np.argmax(prod >= F32(k + 0.5)))
    assert 0 < hi < len(cand)
    return cand[hi - 1], cand[hi]


def _proj(T, X):
    """[R | t] X as the kernels and cv::Mat evaluate it: float products summed left to right, then + t."""
    T = np.asarray(T, F32).reshape(-1)[:12].reshape(3, 4)
    out = []
    for i in range(3):
        s = T[i, 0] * X[..., 0]
        s = s + T[i, 1] * X[..., 1]
        s = s + T[i, 2] * X[..., 2]
        out.append(s + T[i, 3])
    return out


def _nudge(v, span):
    return (np.array([v], F32).view(np.int32) + np.arange(-span, span + 1, dtype=np.int32)).view(F32)


def exact_projection_point(fr: dict, u: float, v: float, z: float = 8.0) -> np.ndarray:
    """A float32 world point whose camera z is exactly z (a power of two, so 1 / z and every product with it
    are exact and the Frame form fx * X * invz + cx and the KeyFrame form fx * (X * invz) + cx agree) and
    whose projected x is exactly the float32 u. Found by searching the neighbouring float32 of Xw; None if
    u cannot be reached (fx * X * invz is rounded at its own magnitude before cx is added, so far from cx only
    multiples of that ulp exist: a fractional min_x may fall between them)."""
    T = np.asarray(fr["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy = (F32(fr[k]) for k in ("fx", "fy", "cx", "cy"))
    Pc = np.array([(u - float(cx)) / float(fx) * z, (v - float(cy)) / float(fy) * z, z])
    X = (T[:, :3].T @ (Pc - T[:, 3])).astype(F32)
    X0, X1, X2 = np.meshgrid(_nudge(X[0], 1500), _nudge(X[1], 6), _nudge(X[2], 12), indexing="ij")
    XX = np.stack([X0, X1, X2], -1)
    pc = _proj(fr["Tcw"], XX)
    uu = fx * pc[0] * (F32(1) / pc[2]) + cx
    hit = np.argwhere((pc[2] == F32(z)) & (uu == F32(u)))
    if not len(hit):
        return None
    return XX[tuple(hit[len(hit) // 2])].copy()


def exact_depth_point(fr: dict, u: float, v: float, negative: bool) -> np.ndarray:
    """A world point whose camera z is exactly 0.0f (negative=False) or the closest float32 below it found
    (negative=True), with camera x, y away from 0 so u, v are +-inf, not NaN."""
    T = np.asarray(fr["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    Pc = np.array([1.0, 0.4, 0.0])
    X = (T[:, :3].T @ (Pc - T[:, 3])).astype(F32)
    X2 = _nudge(X[2], 20000)
    XX = np.stack([np.full_like(X2, X[0]), np.full_like(X2, X[1]), X2], -1)
    z = _proj(fr["Tcw"], XX)[2]
    if negative:
        k = int(np.argmax(np.where(z < 0, z, -np.inf)))
        assert z[k] < 0
    else:
        hit = np.nonzero(z == 0)[0]
        assert len(hit), "no float32 point at z == 0"
        k = int(hit[0])
    return XX[k].copy()


N_EDGE_KP, N_EDGE_MP = 40, 10


def add_edges(p: dict, b) -> dict:
    """Post-process a tracking problem at bounds b:
    keypoints (the last N_EDGE_KP): exactly on min_x / max_x / min_y / max_y, on both sides of the cell
    boundaries (x - min_x) * inv_w = k + 0.5 (track_grid_kernel's roundf), and every fifth keypoint of the frame
    moved to integer pixel coordinates as a level-0 extractor emits them;
    map points (the first N_EDGE_MP): projections exactly on min_x, max_x and on their int truncations (the
    Frame gates are u < min_x || u > max_x, the KeyFrame gates u >= (int)min_x && u < (int)max_x), each with a
    keypoint 0.5 px (min side) / 6 px (max side) inside and a last-frame observation;
    a bound no float32 projection can equal is left out (exact_projection_point): that is the fractional min_x
    10.801 of "tum640", so the Frame gate at u == min_x is met at -27.25 ("neg640", "hd720") and 0.0 ("w752") only; one with camera z == 0 and one just below."""
    fr, mp = p["frame"], {k: v.copy() for k, v in p["map"].items()}
    rng = np.random.default_rng(77)
    kp, desc, ur = fr["keys_un"].copy(), fr["desc"].copy(), fr["u_right"].copy()
    n = len(kp)
    kp["x"][::5] = np.rint(kp["x"][::5])
    kp["y"][::5] = np.rint(kp["y"][::5])
    e0 = n - N_EDGE_KP
    ymid = 0.5 * (b[2] + b[3])
    xs = [b[0], b[1], np.nextafter(F32(b[1]), F32(-1e9))]
    for k in (0, 1, 17, 40, 62, 63):
        xs += list(_cell_edge_x(b, k))
    for j, x in enumerate(xs):
        kp["x"][e0 + j], kp["y"][e0 + j] = x, ymid + 3.0 * j
    j0 = e0 + len(xs)
    for j, y in enumerate((b[2], b[3], np.nextafter(F32(b[3]), F32(-1e9)))):
        kp["x"][j0 + j], kp["y"][j0 + j] = 0.5 * (b[0] + b[1]) + 7.0 * j, y
    j0 += 3
    # exact projections
    us = sorted({float(F32(b[0])), float(F32(b[1])), float(int(b[0])), float(int(b[1]))})
    Ow = np.asarray(fr["Ow"], np.float64)
    last_mp, lk = p["last_mp"].copy(), p["last"]["keys_un"].copy()
    free = np.nonzero(last_mp < 0)[0]
    exact = {}
    for i, u in enumerate(us):
        v = b[2] + 60.0 + 25.0 * i
        X = None
        for v in v + 7.0 * np.arange(8):          # some rows miss (the float32 camera x skips values)
            X = exact_projection_point(fr, u, float(v))
            if X is not None:
                break
        if X is None:
            continue
        d = np.linalg.norm(X.astype(np.float64) - Ow)
        mp["Xw"][i], mp["normal"][i] = X, ((X - Ow) / d).astype(F32)
        mp["max_dist"][i], mp["min_dist"][i] = 1.2 * 0.999 * d, 0.3 * d
        mp["flags"][i] = synth.MP_HAS_OBS
        k = j0 + i
        inside = u + 0.5 if abs(u - b[0]) < 1.0 else u - 6.0     # the last half cell before max_x is off the grid
        kp["x"][k], kp["y"][k], kp["octave"][k] = inside, v, 1
        desc[k] = synth._flip_bits(rng, mp["desc"][i], 5)
        ur[k] = -1.0
        last_mp[last_mp == i] = -1
        last_mp[free[i]] = i
        lk["octave"][free[i]] = 1
        exact[u] = (i, k)
    for i, neg in ((len(us), False), (len(us) + 1, True)):
        mp["Xw"][i] = exact_depth_point(fr, 0, 0, neg)
        mp["flags"][i] = synth.MP_HAS_OBS
        last_mp[last_mp == i] = -1
        last_mp[free[i]] = i
    frame = dict(fr, keys_un=kp, desc=desc, u_right=ur)
    blocked = None if p.get("kp_blocked") is None else p["kp_blocked"].copy()
    if blocked is not None:
        blocked[e0:] = 0
    lo = p["last_outlier"].copy()
    lo[free[:len(us) + 2]] = 0
    return dict(p, frame=frame, map=mp, last=dict(p["last"], keys_un=lk), last_mp=last_mp, last_outlier=lo,
                kp_blocked=blocked, exact=exact, z_points=(len(us), len(us) + 1))


def bounds_problem(oracle_mod, name: str, seed: int = 70, reloc: bool = False, n_kp: int = 1000, n_mp: int = 1500):
    """synth.tracking_problem (or reloc_problem) at the camera's image size, min_x..max_y of the frame and the
    last frame replaced by camera_bounds(name) (fractional and non-zero for "tum640", negative minima for
    "neg640" / "hd720"), plus add_edges(): grid_window, track_grid_kernel and every bounds gate read values
    other than 0, W, 0, H, and keypoints fall outside the grid on all four sides."""
    W, H, _ = CAMERAS[name]
    b = camera_bounds(oracle_mod, name)
    gen = synth.reloc_problem if reloc else synth.tracking_problem
    p = gen(seed, n_kp=n_kp, n_mp=n_mp, W=W, H=H, n_last=800)
    p = dict(p, frame=_with_bounds(p["frame"], b), last=_with_bounds(p["last"], b))
    return sim3_stage(add_edges(p, b), scale=1.37)


def bounds_pair_problem(oracle_mod, name: str, seed: int = 80, n: int = 900, n_points: int = 800):
    """synth.sim3_pair_problem (ORBmatcher::SearchBySim3) at the camera's size and bounds, every fifth keypoint at
    integer pixels: both keyframes' IsInImage / GetFeaturesInArea use the int-truncated bounds."""
    W, H, _ = CAMERAS[name]
    b = camera_bounds(oracle_mod, name)
    p = synth.sim3_pair_problem(seed, n=n, n_points=n_points, W=W, H=H)
    out = dict(p)
    for k in ("kf1", "kf2"):
        kp = p[k]["keys_un"].copy()
        kp["x"][::5] = np.rint(kp["x"][::5])
        kp["y"][::5] = np.rint(kp["y"][::5])
        out[k] = _with_bounds(dict(p[k], keys_un=kp), b)
    return out


# ---------------------------------------------------------------------------------------------
# d. decisions at equality: isolated spots, one map point each with hand-made candidates
# ---------------------------------------------------------------------------------------------
def spots_problem(spots, seed: int = 9) -> dict:
    """One map point per spot on a 70 px lattice (12 m deep, so windows never overlap), each with its own
    keypoints: spot = {"level": predicted level L of the map point (default 1), "kps": [(dx, dy, octave,
    flipped bits, angle)], "last_angle", "last_octave" (default L), "obs" (default True), "on_cell_edge"}. Keypoint
    descriptors are the map point's with exactly `flipped bits` random bits flipped (synth._flip_bits), so
    every Hamming distance is known. The last frame / candidate keyframe sees map point i in its keypoint i.
    Returns the tracking-problem dict staged for the Sim3 searches too, plus "spots" with "kp" index lists."""
    p = synth.tracking_problem(1, n_kp=64, n_mp=20)
    fr = p["frame"]
    rng = np.random.default_rng(seed)
    T = np.asarray(fr["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    Ow = np.asarray(fr["Ow"], np.float64)
    fx, fy, cx, cy = (float(fr[k]) for k in ("fx", "fy", "cx", "cy"))
    n_mp, n_kp = len(spots), sum(len(s["kps"]) for s in spots)
    assert n_mp <= 75
    kp = np.zeros(n_kp, synth.TRACK_KP_DTYPE)
    desc = np.zeros((n_kp, 32), np.uint8)
    mp = {"Xw": np.zeros((n_mp, 3), F32), "normal": np.zeros((n_mp, 3), F32), "max_dist": np.zeros(n_mp, F32),
          "min_dist": np.zeros(n_mp, F32), "desc": rng.integers(0, 256, (n_mp, 32), dtype=np.uint8),
          "flags": np.zeros(n_mp, np.uint8)}
    lk = np.zeros(n_mp, synth.TRACK_KP_DTYPE)
    meta, k = [], 0
    for i, s in enumerate(spots):
        L = s.get("level", 1)
        u, v, z = 100.0 + 70.0 * (i % 15), 60.0 + 70.0 * (i // 15), 12.0
        if s.get("on_cell_edge"):       # on a grid column boundary: keypoints left and right of it are in two cells
            cw = (fr["max_x"] - fr["min_x"]) / GRID_COLS
            u = (np.floor(u / cw) + 0.5) * cw
        Pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        X = (T[:, :3].T @ (Pc - T[:, 3])).astype(F32)
        d = np.linalg.norm(X.astype(np.float64) - Ow)
        mp["Xw"][i], mp["normal"][i] = X, ((X - Ow) / d).astype(F32)
        mp["max_dist"][i] = (1.2 ** L) * 0.999 * d
        mp["min_dist"][i] = 0.3 * d
        mp["flags"][i] = synth.MP_HAS_OBS if s.get("obs", True) else 0
        idx = []
        for dx, dy, o, nflip, ang in s["kps"]:
            kp[k] = (u + dx, v + dy, 31.0 * 1.2 ** o, ang, 0, o, -1)
            desc[k] = synth._flip_bits(rng, mp["desc"][i], nflip)
            idx.append(k)
            k += 1
        lk[i] = (0, 0, 31.0, s.get("last_angle", 0.0), 0, s.get("last_octave", L), -1)
        meta.append(dict(s, kp=idx, u=u, v=v))
    frame = dict(fr, keys_un=kp, desc=desc, u_right=np.full(n_kp, -1, F32))
    last = dict(p["last"], keys_un=lk, u_right=np.full(n_mp, -1, F32), desc=np.zeros((n_mp, 32), np.uint8))
    out = dict(p, frame=frame, map=mp, last=last, last_mp=np.arange(n_mp, dtype=np.int32),
               last_outlier=np.zeros(n_mp, np.uint8), kp_blocked=None, spots=meta)
    return sim3_stage(out)


def as_pair(p: dict) -> dict:
    """A spots problem as a SearchBySim3 pair: both keyframes are the frame itself at the same pose (s12 = 1,
    R12 = I, t12 = 0), the first keypoint of every spot holds the spot's map point in both, so the two
    projections agree whenever that keypoint's distance passes TH_HIGH."""
    n = len(p["frame"]["keys_un"])
    mpk = np.full(n, -1, np.int32)
    for i, s in enumerate(p["spots"]):
        mpk[s["kp"][0]] = i
    return {"kf1": p["frame"], "kf1_mp": mpk, "kf2": p["frame"], "kf2_mp": mpk.copy(), "map": p["map"],
            "s12": np.float32(1.0), "R12": np.eye(3, dtype=np.float32), "t12": np.zeros(3, np.float32),
            "matches12": np.full(n, -1, np.int32)}


GATE_DISTS = (49, 50, 51, 63, 64, 65, 99, 100, 101)
RATIOS = ((0.75, 75, 100), (0.8, 80, 100), (0.9, 90, 100), (0.6, 60, 100))


def gates_problem() -> dict:
    """One candidate per map point at Hamming distance exactly GATE_DISTS[i]: TH_HIGH 100 (local, frame,
    SearchBySim3), TH_LOW 50 (Sim3 projection), ORBdist 64 / 100 (relocalisation), each with the value at the
    gate, one below and one above. Fuse reports the distance itself."""
    return spots_problem([{"kps": [(0.4, -0.3, 1, g, 10.0)]} for g in GATE_DISTS])


def ratio_problem() -> dict:
    """SearchByProjection(F, vpMapPoints)'s `bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2` at float
    equality: for each (nnratio, d1, d2) of RATIOS one spot with best and second on the same level and one
    with them on different levels (spot 2k / 2k + 1). Run at each of the four nnratio values."""
    spots = []
    for _, d1, d2 in RATIOS:
        spots.append({"kps": [(0.4, -0.3, 1, d1, 0.0), (-0.5, 0.2, 1, d2, 0.0)]})
        spots.append({"kps": [(0.4, -0.3, 1, d1, 0.0), (-0.5, 0.2, 0, d2, 0.0)]})
    return spots_problem(spots)


def ties_problem() -> dict:
    """Two and three candidates at the same minimum distance in one window, listed so that keypoint index order
    and grid column order disagree (the spots sit on a column boundary): first in the reference's candidate order (grid column, row, insertion) wins in every
    projection search; on one level the local search's ratio test rejects the tie instead."""
    t = [(0.9, 0.1, 40), (-0.8, -0.2, 40), (0.1, 0.7, 40)]
    spots = []
    for n in (2, 3):
        spots.append({"kps": [(dx, dy, 1, d, 0.0) for dx, dy, d in t[:n]]})                       # same level
        spots.append({"kps": [(dx, dy, 1 - (j % 2), d, 0.0) for j, (dx, dy, d) in enumerate(t[:n])]})
        spots.append({"kps": [(dx, dy, 1, d, 0.0) for dx, dy, d in t[:n]] + [(0.0, -0.6, 1, 70, 0.0)]})
    return spots_problem([dict(s, on_cell_edge=True) for s in spots])


def ref_order(fr: dict, idx):
    """Candidate order of GetFeaturesInArea: grid column, then row, then insertion (= keypoint index)."""
    b = (fr["min_x"], fr["max_x"], fr["min_y"], fr["max_y"])
    kp = fr["keys_un"]
    px, py, _ = pos_in_grid(kp["x"][idx], kp["y"][idx], b)
    return [i for _, _, i in sorted(zip(px.tolist(), py.tolist(), list(idx)))]


def hamming(a, b) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def local_decision(p: dict, i: int, nnratio: float):
    """ORBmatcher.cc:78-176 on an isolated spot: the keypoint index map point i takes, or -1."""
    s, fr = p["spots"][i], p["frame"]
    L = s.get("level", 1)
    best = best2 = 256
    lvl = lvl2 = idx = -1
    for k in ref_order(fr, s["kp"]):
        o = int(fr["keys_un"]["octave"][k])
        if o < L - 1 or o > L:
            continue
        d = hamming(p["map"]["desc"][i], fr["desc"][k])
        if d < best:
            best2, lvl2, best, lvl, idx = best, lvl, d, o, k
        elif d < best2:
            best2, lvl2 = d, o
    if best <= 100:
        if lvl == lvl2 and F32(best) > F32(nnratio) * F32(best2):
            return -1
        return idx
    return -1


def first_min_decision(p: dict, i: int, gate: int, lo: int = -1, hi: int = 1):
    """The other projection searches on an isolated spot: first minimum in candidate order over octaves
    [L + lo, L + hi], accepted if <= gate. Returns (keypoint index or -1, distance)."""
    s, fr = p["spots"][i], p["frame"]
    L = s.get("level", 1)
    best, idx = 256, -1
    for k in ref_order(fr, s["kp"]):
        o = int(fr["keys_un"]["octave"][k])
        if o < L + lo or o > L + hi:
            continue
        d = hamming(p["map"]["desc"][i], fr["desc"][k])
        if d < best:
            best, idx = d, k
    return (idx if best <= gate else -1), best


def rot_bin(a1: float, a2: float) -> int:
    """ORBmatcher.cc:1872-1878: rot = a1 - a2 (+360 if negative), bin = round(rot * factor), 30 -> 0, evaluated
    on the float32 product (round half away from zero = floor(x + 0.5) for x >= 0)."""
    rot = F32(a1) - F32(a2)
    if rot < 0:
        rot = F32(rot + F32(360.0))
    b = int(np.floor(float(F32(rot * F32(HISTO_LENGTH / F32(360.0)))) + 0.5))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(counts):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2076-2118) -> the kept bins."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if m2 < F32(0.1) * F32(m1):
        i2 = i3 = -1
    elif m3 < F32(0.1) * F32(m1):
        i3 = -1
    return {i1, i2, i3} - {-1}


# (query angle, candidate angle) lists: rot = query - candidate
def _rep(pair, n):
    return [pair] * n


ROT_SETS = {
    # three full bins (0, 1, 2) and single matches exactly on bin edges 6 + 12 k, in 354..360, and negative
    "edges": _rep((50.0, 50.0), 8) + _rep((62.0, 50.0), 8) + _rep((74.0, 50.0), 8) +
             [(56.0, 50.0), (68.0, 50.0), (80.0, 50.0), (92.0, 50.0), (44.0, 50.0), (32.0, 50.0), (44.0, 62.0),
              (354.0, 0.0), (357.5, 0.0), (359.99, 0.0), (360.0, 0.0), (10.0, 20.0), (0.0, 359.5), (5.999, 0.0),
              (6.0, 0.0), (6.001, 0.0), (18.0, 0.0), (30.0, 0.0), (342.0, 0.0), (0.0, 6.0), (0.0, 18.0)],
    # four bins tie for the maximum: the first three in bin order stay
    "tie_max": _rep((100.0, 76.0), 5) + _rep((100.0, 40.0), 5) + _rep((100.0, 4.0), 5) + _rep((200.0, 80.0), 5),
    # max2 == 0.1f * max1 (20 and 2): the second bin stays; max3 = 1 goes
    "ten_percent": _rep((100.0, 64.0), 20) + _rep((100.0, 40.0), 2) + [(100.0, 4.0)],
    # 30, 2, 2: max2 < 0.1f * 30, both go
    "below": _rep((100.0, 64.0), 30) + _rep((100.0, 40.0), 2) + _rep((100.0, 4.0), 2),
    "one_bin": _rep((100.0, 64.0), 12),
}


def rot_problem(name: str) -> dict:
    """One sure match (distance 10) per spot with the last keypoint's and the current keypoint's angles of
    ROT_SETS[name]: the rotation histogram of SearchByProjection(CurrentFrame, LastFrame) and of the
    relocalisation search gets exactly those counts."""
    return spots_problem([{"kps": [(0.3, 0.2, 1, 10, a2)], "last_angle": a1} for a1, a2 in ROT_SETS[name]])


def rot_survivors(pairs):
    bins = [rot_bin(a1, a2) for a1, a2 in pairs]
    keep = three_maxima(np.bincount(bins, minlength=HISTO_LENGTH))
    return [b in keep for b in bins], bins


def predict_scale_problem() -> dict:
    """MapPoint::PredictScale with max_dist / dist == 1.2f^k exactly in float (k = 0..7: ceil(log(ratio) /
    log(1.2f)) lands on or next to an integer), a ratio below 1 (clamps to level 0) and of 1.2^9.5 (clamps
    to nlevels - 1); RadiusByViewingCos with viewCos the two float32 around 0.998; viewCos exactly 0.5f, the
    isInFrustum limit. Spots carry "ratio" / "view_cos" = the float32 value the kernel must see."""
    spots = [{"kps": [(0.3, 0.2, min(k, 7), 10, 0.0)], "level": k} for k in range(8)]
    spots += [{"kps": [(0.3, 0.2, 0, 10, 0.0)], "level": 0}, {"kps": [(0.3, 0.2, 7, 10, 0.0)], "level": 7}]
    # radius 2.5 vs 4.0 at level 1: a keypoint 3.5 px away is inside only with the wide radius
    spots += [{"kps": [(3.5, 0.2, 1, 10, 0.0)]} for _ in range(5)]
    p = spots_problem(spots)
    mp = {k: v.copy() for k, v in p["map"].items()}
    Ow = np.asarray(p["frame"]["Ow"], F32)
    sf = np.asarray(p["frame"]["scale_factors"], F32)

    def dist_of(i):
        PO = (mp["Xw"][i] - Ow).astype(np.float64)      # float subtraction, double sum of squares (cv::norm)
        return F32(np.sqrt((PO * PO).sum())), PO

    meta = [dict(s) for s in p["spots"]]
    for k in range(8):
        d, _ = dist_of(k)
        c = _nudge(F32(sf[k] * d), 16)
        hit = c[(c / d) == sf[k]]
        assert len(hit), k
        mp["max_dist"][k], mp["min_dist"][k] = hit[0], F32(0.3) * d
        meta[k]["ratio"] = float(sf[k])
    d, _ = dist_of(8)
    mp["max_dist"][8], mp["min_dist"][8] = F32(0.9) * d, F32(0.3) * d
    d, _ = dist_of(9)
    mp["max_dist"][9], mp["min_dist"][9] = F32(1.2 ** 9.5) * d, F32(0.3) * d
    lo = np.nextafter(F32(0.998), F32(0))
    for i, target in zip(range(10, 15), (F32(0.5), lo, np.nextafter(lo, F32(1)), np.nextafter(F32(0.5), F32(1)),
                                         F32(1.0))):
        d, PO = dist_of(i)
        # normal = PO * c plus a perpendicular part that does not change the dot product: only c matters
        c0 = float(target) * float(d) / float((PO * PO).sum())
        found = False
        for c in _nudge(F32(c0), 200):
            nrm = (PO * float(c)).astype(F32)
            dot = 0.0
            for a, bb in zip(PO, nrm.astype(np.float64)):
                dot = dot + a * bb
            if F32(dot / float(d)) == target:
                found = True
                break
        assert found, i
        mp["normal"][i] = nrm
        meta[i]["view_cos"] = float(target)
    return dict(p, map=mp, spots=meta)


# ---- BoW micro problems: one node per cell, hand-made candidates at chosen positions of the node
def bow_cells_problem(cells, seed: int = 4) -> dict:
    """cells[c] = {"nb": B-features in node c, "queries": [{"cands": {position in the node: distance}, "angle",
    "from": (earlier query, position)}], "b_angle": {position: angle}}. Node c holds the cell's A-features
    (the queries, in order) and nb B-features; positions without a candidate hold random descriptors.
    "from" makes the query's descriptor that B-feature's with `distance` bits flipped (so two queries
    compete for one position); otherwise candidates are the query's descriptor with `distance` flipped bits.
    Both sides carry good map points and the keypoint positions are random: these problems are for the two
    SearchByBoW forms only (SearchForTriangulation skips every A-feature that holds a map point; its gate and
    histogram cases are tri_gate_rot_problem)."""
    rng = np.random.default_rng(seed)
    base = synth.bow_match_problem(3, n=64, n_points=50)
    na = sum(len(c["queries"]) for c in cells)
    nb = sum(c["nb"] for c in cells)

    def blank(n):
        k = np.zeros(n, synth.TRACK_KP_DTYPE)
        k["x"], k["y"], k["size"], k["class_id"] = rng.uniform(0, 1241, n), rng.uniform(0, 376, n), 31.0, -1
        return k

    kA, kB = blank(na), blank(nb)
    dA, dB = np.zeros((na, 32), np.uint8), rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    nodesA, nodesB = np.zeros(na, np.int64), np.zeros(nb, np.int64)
    ia = ib0 = 0
    meta = []
    for c, cell in enumerate(cells):
        nodesB[ib0:ib0 + cell["nb"]] = c
        for pos, ang in cell.get("b_angle", {}).items():
            kB["angle"][ib0 + pos] = ang
        qs = []
        for q in cell["queries"]:
            nodesA[ia] = c
            kA["angle"][ia] = q.get("angle", 0.0)
            cands = dict(q["cands"])
            if "from" in q:
                pos = q["from"]
                dA[ia] = synth._flip_bits(rng, dB[ib0 + pos], cands.pop(pos))
            else:
                dA[ia] = rng.integers(0, 256, 32, dtype=np.uint8)
            for pos, dist in cands.items():
                dB[ib0 + pos] = synth._flip_bits(rng, dA[ia], dist)
            qs.append(ia)
            ia += 1
        meta.append({"a": qs, "b0": ib0, "nb": cell["nb"]})
        ib0 += cell["nb"]

    def kf(src, k, d, nodes, n):
        fvn, fvs, fvf = synth._fv_from_nodes(nodes)
        return dict(src, keys_un=k, desc=d, u_right=np.full(n, -1, F32), mp=np.arange(n, dtype=np.int32),
                    mp_bad=np.zeros(n, np.uint8), fv_nodes=fvn, fv_start=fvs, fv_features=fvf)

    return dict(base, A=kf(base["A"], kA, dA, nodesA, na), B=kf(base["B"], kB, dB, nodesB, nb), cells=meta)


def bow_decisions(p: dict, nnratio: float, strict: bool):
    """SearchByBoW on the cells, sequentially (ORBmatcher.cc:236-353 / 760-903): per A-feature the B index it
    takes or -1. strict = the (KeyFrame, KeyFrame) form's bestDist1 < TH_LOW."""
    A, B = p["A"], p["B"]
    out = np.full(len(A["keys_un"]), -1, np.int64)
    for cell in p["cells"]:
        taken = set()
        for ia in cell["a"]:
            b1 = b2 = 256
            idx = -1
            for pos in range(cell["nb"]):
                if pos in taken:
                    continue
                d = hamming(A["desc"][ia], B["desc"][cell["b0"] + pos])
                if d < b1:
                    b2, b1, idx = b1, d, pos
                elif d < b2:
                    b2 = d
            if (b1 < 50 if strict else b1 <= 50) and F32(b1) < F32(nnratio) * F32(b2):
                taken.add(idx)
                out[ia] = cell["b0"] + idx
    return out


BOW_RATIOS = RATIOS + ((0.75, 45, 60), (0.8, 40, 50), (0.9, 45, 50), (0.6, 30, 50), (0.7, 35, 50))


def bow_equality_problem() -> dict:
    """Gates 49 / 50 / 51 alone in a node (TH_LOW: <= in SearchByBoW(KF, F), < in (KF, KF)); the ratio test
    bestDist1 < mfNNratio * bestDist2 at float equality (RATIOS, rejected by the gate anyway, and the same
    products with d1 <= 50); ties for the best in different lanes (positions 3, 10), in one lane (5, 69) and
    three ways (1, 65, 129): best == second, so the ratio test rejects; a tie for second place (6, 70) behind
    a best at position 100; and two queries after one position >= 64 (70): the second must see it claimed."""
    cells = [{"nb": 1, "queries": [{"cands": {0: g}}]} for g in (49, 50, 51)]
    cells += [{"nb": 2, "queries": [{"cands": {0: d1, 1: d2}}]} for _, d1, d2 in BOW_RATIOS]
    cells += [{"nb": 70, "queries": [{"cands": {3: 30, 10: 30}}]},
              {"nb": 130, "queries": [{"cands": {5: 30, 69: 30}}]},
              {"nb": 130, "queries": [{"cands": {1: 30, 65: 30, 129: 30}}]},
              {"nb": 130, "queries": [{"cands": {100: 20, 6: 45, 70: 45}}]},
              {"nb": 130, "queries": [{"cands": {70: 20, 6: 48}}, {"cands": {70: 10, 100: 25}, "from": 70}]}]
    return bow_cells_problem(cells)


def bow_rot_problem(name: str) -> dict:
    """One sure match (distance 10, alone in its node) per pair of ROT_SETS[name]: the BoW matchers' rotation
    histogram (rot = KF angle - F angle) with those counts."""
    return bow_cells_problem([{"nb": 1, "queries": [{"cands": {0: 10}, "angle": a1}], "b_angle": {0: a2}}
                              for a1, a2 in ROT_SETS[name]])


TRI_REJECTED = 8


def tri_gate_rot_problem(pairs, name: str, seed: int = 31):
    """SearchForTriangulation at its gate and through its rotation histogram, on geometry it accepts: `pairs` are
    the oracle's pairs (ia, ib) of bow_case("one") (one 600-feature node, epipolar and epipole gates passed).
    Pair k < len(ROT_SETS[name]) gets B's descriptor = A's with exactly 50 (even k) or 49 (odd k) flipped bits
    and the angles ROT_SETS[name][k]; the next TRI_REJECTED pairs get 51 flipped bits (`dist > TH_LOW` rejects,
    ORBmatcher.cc:1014). Every other B-feature without a map point is given one, so only these B-features are
    candidates, and a descriptor 49..51 bits from one A-feature is ~128 bits from every other: the result is
    pair k for every k below len(ROT_SETS[name]), minus those the rotation check removes.
    Returns (problem, used pairs, flipped bits per used pair)."""
    p = bow_case("one")
    rot = ROT_SETS[name]
    n_used = len(rot) + TRI_REJECTED
    assert len(pairs) >= n_used
    used = [(int(a), int(b)) for a, b in pairs[:n_used]]
    rng = np.random.default_rng(seed)
    A = dict(p["A"], keys_un=p["A"]["keys_un"].copy())
    B = dict(p["B"], keys_un=p["B"]["keys_un"].copy(), desc=p["B"]["desc"].copy(), mp=p["B"]["mp"].copy(),
             mp_bad=p["B"]["mp_bad"].copy())
    keep = np.zeros(len(B["mp"]), bool)
    keep[[b for _, b in used]] = True
    B["mp"][(B["mp"] < 0) & ~keep] = 0
    dists = []
    for k, (ia, ib) in enumerate(used):
        d = (50 if k % 2 == 0 else 49) if k < len(rot) else 51
        B["desc"][ib] = synth._flip_bits(rng, A["desc"][ia], d)
        if k < len(rot):
            A["keys_un"]["angle"][ia], B["keys_un"]["angle"][ib] = rot[k]
        dists.append(d)
    return dict(p, A=A, B=B), used, dists


# ---------------------------------------------------------------------------------------------
# e. capacity
# ---------------------------------------------------------------------------------------------
def one_cell_problem(n_kp: int = 8192, n_mp: int = 300, seed: int = 12) -> dict:
    """All n_kp keypoints inside one grid cell (19 x 7 px around one place), n_mp map points projecting
    there: every window holds thousands of candidates, so the position half of the dist << 16 | position key
    runs up to n_kp - 1 and one cell's CSR range spans the whole sorted array."""
    p = synth.tracking_problem(seed, n_kp=n_kp, n_mp=n_mp, n_last=n_mp)
    fr = p["frame"]
    rng = np.random.default_rng(seed)
    b = (fr["min_x"], fr["max_x"], fr["min_y"], fr["max_y"])
    cw, ch = (b[1] - b[0]) / GRID_COLS, (b[3] - b[2]) / GRID_ROWS
    x0, y0 = b[0] + 30 * cw, b[2] + 20 * ch               # centre of cell (30, 20)
    kp = fr["keys_un"].copy()
    kp["x"] = x0 + rng.uniform(-0.45, 0.45, n_kp) * cw
    kp["y"] = y0 + rng.uniform(-0.45, 0.45, n_kp) * ch
    kp["octave"] = rng.integers(0, 3, n_kp)
    T = np.asarray(fr["Tcw"], np.float64).reshape(-1)[:12].reshape(3, 4)
    Ow = np.asarray(fr["Ow"], np.float64)
    fx, fy, cx, cy = (float(fr[k]) for k in ("fx", "fy", "cx", "cy"))
    z = rng.uniform(6, 20, n_mp)
    u, v = x0 + rng.uniform(-3, 3, n_mp), y0 + rng.uniform(-2, 2, n_mp)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    X = (Pc - T[:, 3]) @ T[:, :3]
    d = np.linalg.norm(X - Ow, axis=1)
    desc = fr["desc"].copy()
    mdesc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    for m in range(n_mp):                                    # a few keypoints resemble each map point
        for k in rng.integers(0, n_kp, 3):
            desc[k] = synth._flip_bits(rng, mdesc[m], int(rng.integers(0, 60)))
    mp = {"Xw": X.astype(F32), "normal": ((X - Ow) / d[:, None]).astype(F32), "max_dist": (1.2 * 0.999 * d).astype(F32),
          "min_dist": (0.3 * d).astype(F32), "desc": mdesc, "flags": np.full(n_mp, synth.MP_HAS_OBS, np.uint8)}
    lk = p["last"]["keys_un"].copy()
    lk["octave"] = 1
    return sim3_stage(dict(p, frame=dict(fr, keys_un=kp, desc=desc, u_right=np.full(n_kp, -1, F32)), map=mp,
                           last=dict(p["last"], keys_un=lk), last_mp=np.arange(n_mp, dtype=np.int32),
                           last_outlier=np.zeros(n_mp, np.uint8), kp_blocked=None))


# ---------------------------------------------------------------------------------------------
# registries: each problem is built once per process and never modified by a test
# ---------------------------------------------------------------------------------------------
ROT_NAMES = tuple(ROT_SETS)
BOW_CASES = {
    "mod3": lambda: regroup(synth.bow_match_problem(3, n=600, n_points=480), "mod3"),
    "one": lambda: regroup(synth.bow_match_problem(4, n=600, n_points=480), "one"),
    "skewed": lambda: regroup(synth.bow_match_problem(6, n=600, n_points=480), "skewed"),
    "sizes": node_sizes_problem,
    "one4096": lambda: regroup(synth.bow_match_problem(5, n=4096, n_points=3276), "one"),
    "quant1": lambda: quantise_bow(bow_case("mod3"), 1),
    "quant2": lambda: quantise_bow(bow_case("mod3"), 2),
    "quant4": lambda: quantise_bow(bow_case("one"), 4),
    "equality": bow_equality_problem,
    **{"rot_" + k: functools.partial(bow_rot_problem, k) for k in ROT_SETS},
}


@functools.lru_cache(maxsize=None)
def bow_case(name: str) -> dict:
    return BOW_CASES[name]()


def bow_tie_problem(oracle_mod, mode: str, stride: int, count: int = 8):
    """bow_case("one") with `count` of the oracle's matches of `mode` ("bow", "bowkf", "tri") given a second,
    identical B-candidate `stride` positions later (duplicate_b). Returns (problem, [(ia, ib)])."""
    p = bow_case("one")
    A, B = p["A"], p["B"]
    n = len(B["keys_un"])
    if mode == "tri":
        got = [tuple(int(v) for v in r) for r in oracle_mod.search_for_triangulation(p)]
    elif mode == "bowkf":
        _, m = oracle_mod.search_by_bow_kf(p)
        got = [(ia, int(np.nonzero((B["mp"] == m[ia]))[0][0])) for ia in np.nonzero(m >= 0)[0]]
    else:
        _, m = oracle_mod.search_by_bow(p)
        got = []
        for ib in np.nonzero(m >= 0)[0]:
            ia = np.nonzero((A["mp"] == m[ib]) & (A["mp_bad"] == 0))[0]
            if len(ia) == 1:
                got.append((int(ia[0]), int(ib)))
    used = {ib for _, ib in got}
    pairs = []
    for ia, ib in got:
        t = ib + stride
        if t >= n or t in used or ib in {q + stride for _, q in pairs} or len(pairs) >= count:
            continue
        if mode == "bowkf" and int((B["mp"] == B["mp"][ib]).sum()) != 1:
            continue
        used.add(t)
        pairs.append((ia, ib))
    return duplicate_b(p, pairs, stride), pairs


_TRI = {}


def tri_case(oracle_mod, name: str):
    """tri_gate_rot_problem on the oracle's pairs of bow_case("one") without the rotation check."""
    if name not in _TRI:
        _TRI[name] = tri_gate_rot_problem(oracle_mod.search_for_triangulation(bow_case("one"), False, False), name)
    return _TRI[name]


TRACK_CASES = {
    **{"crowd_" + k: functools.partial(crowd, k) for k in CROWDS},
    "gates": gates_problem, "ratio": ratio_problem, "ties": ties_problem, "scale": predict_scale_problem,
    **{"rot_" + k: functools.partial(rot_problem, k) for k in ROT_SETS},
    "quant1": lambda: sim3_stage(quantise_track(synth.tracking_problem(5, n_kp=1000, n_mp=1500, n_last=800), 1), 1.21),
    "quant2": lambda: sim3_stage(quantise_track(synth.tracking_problem(5, n_kp=1000, n_mp=1500, n_last=800), 2), 1.21),
    "quant4": lambda: sim3_stage(quantise_track(synth.tracking_problem(5, n_kp=1000, n_mp=1500, n_last=800), 4), 1.21),
    "one_cell": one_cell_problem,
    "cap8192": lambda: sim3_stage(synth.tracking_problem(8, n_kp=8192, n_mp=9000, n_last=8192), 1.21),
    "cap8191": lambda: sim3_stage(synth.tracking_problem(9, n_kp=8191, n_mp=3000, n_last=8191), 1.21),
    "cap4097": lambda: sim3_stage(synth.tracking_problem(10, n_kp=4097, n_mp=3000, n_last=4097), 1.21),
    "cap1": lambda: sim3_stage(synth.tracking_problem(11, n_kp=1, n_mp=50, n_last=1), 1.21),
}


@functools.lru_cache(maxsize=None)
def track_case(name: str) -> dict:
    return TRACK_CASES[name]()


_BOUNDS = {}


def bounds_case(oracle_mod, name: str, kind: str = "track") -> dict:
    """kind: "track" (tracking_problem), "reloc" (reloc_problem) or "pair" (sim3_pair_problem) at CAMERAS[name]."""
    key = (name, kind)
    if key not in _BOUNDS:
        _BOUNDS[key] = (bounds_pair_problem(oracle_mod, name) if kind == "pair" else
                        bounds_problem(oracle_mod, name, seed=71 if kind == "reloc" else 70, reloc=kind == "reloc"))
    return _BOUNDS[key]


def quantise_pair(p: dict, nbytes: int) -> dict:
    """quantise_track for a sim3_pair_problem: both keyframes' and the map points' descriptors."""
    def q(d):
        d = d.copy()
        d[:, nbytes:] = 0
        return d
    return dict(p, kf1=dict(p["kf1"], desc=q(p["kf1"]["desc"])), kf2=dict(p["kf2"], desc=q(p["kf2"]["desc"])),
                map=dict(p["map"], desc=q(p["map"]["desc"])))


PAIR_CASES = {
    "gates": lambda: as_pair(track_case("gates")), "ties": lambda: as_pair(track_case("ties")),
    "quant2": lambda: quantise_pair(synth.sim3_pair_problem(81, n=700, n_points=600), 2),
    "cap8192": lambda: synth.sim3_pair_problem(88, n=8192, n_points=7000),
}


@functools.lru_cache(maxsize=None)
def pair_case(name: str) -> dict:
    return PAIR_CASES[name]()
