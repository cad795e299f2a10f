"""Hand-built tracking-matcher cases shared by the CPU and GPU tests."""
import numpy as np

from orbslam2_amd import synth

CROWD_PLACES = ((1.0, 0.5, 12.0), (-3.0, -0.8, 15.0), (4.0, 1.2, 9.0))   # camera-frame positions of crowds


def crowd_problem(n_kp_near: int = 12, n_mp: int = 20, lead: int = 0, tail: int = 0, members=None,
                  no_obs_every: int = 0):
    """n_mp map points at one 3D location competing for n_kp_near keypoints around its
    projection. Keypoint j's descriptor is the map descriptor with 8*j flipped bits and
    octaves alternate 0/1 (so the ratio test never fires: best and second are on different
    levels). The greedy order then assigns keypoint j to map point j while the best distance
    stays <= TH_HIGH -- after 4 claims every map point's kept top-4 candidates are claimed,
    so this exercises the GPU resolve kernels' exact rescan fallback.

    The defaults give the original single crowd in queries 0..n_mp-1. Generalised:
    * lead / tail: that many ordinary map points (of synth.tracking_problem, same camera pose) before /
      after the crowd in query order, so the crowd can sit anywhere in the resolve kernels' 64-query
      windows;
    * members: a list of query-position lists, one per crowd (crowd c at CROWD_PLACES[c], its own
      base descriptor and n_kp_near keypoints c * n_kp_near + j); every other position below
      max(member) + 1 + tail is an ordinary point. Overrides n_mp / lead;
    * no_obs_every = k: every k-th member of each crowd (members 1, 1 + k, ...) has flags == 0, so it
      takes a keypoint without blocking it and the next member overwrites the owner.
    The result carries "crowd" = {"members", "n_near"} for crowd_expected_owner()."""
    p = synth.tracking_problem(1, n_kp=64, n_mp=20)
    fr = p["frame"]
    rng = np.random.default_rng(3)
    R = np.asarray(fr["Tcw"], np.float64)[:, :3]
    t = np.asarray(fr["Tcw"], np.float64)[:, 3]
    if members is None:
        members = [list(range(lead, lead + n_mp))]
    members = [list(map(int, m)) for m in members]
    assert len(members) <= len(CROWD_PLACES) and len(members) * n_kp_near <= 64
    n_total = max(max(m) for m in members) + 1 + tail
    flat = [q for m in members for q in m]
    assert len(set(flat)) == len(flat)
    kp = fr["keys_un"].copy()
    kp["x"] = rng.uniform(0, 1241, len(kp))
    kp["y"] = rng.uniform(0, 376, len(kp))
    desc = fr["desc"].copy()
    Ow = np.asarray(fr["Ow"], np.float64)
    n_fill = n_total - len(flat)
    mp = None
    if n_fill:
        fill = synth.tracking_problem(1, n_kp=64, n_mp=max(20, n_fill))["map"]
        mp = {k: np.zeros((n_total,) + v.shape[1:], v.dtype) for k, v in fill.items()}
        pos = np.setdiff1d(np.arange(n_total), flat)
        for k, v in fill.items():
            mp[k][pos] = v[:n_fill]
    for c, mem in enumerate(members):
        Pc = np.array(CROWD_PLACES[c])
        Xw = R.T @ (Pc - t)
        u = fr["fx"] * Pc[0] / Pc[2] + fr["cx"]
        v = fr["fy"] * Pc[1] / Pc[2] + fr["cy"]
        k0 = c * n_kp_near
        kp["x"][k0:k0 + n_kp_near] = u + rng.uniform(-1.5, 1.5, n_kp_near)
        kp["y"][k0:k0 + n_kp_near] = v + rng.uniform(-1.5, 1.5, n_kp_near)
        kp["octave"][k0:k0 + n_kp_near] = np.arange(n_kp_near) % 2
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for j in range(n_kp_near):
            desc[k0 + j] = synth._flip_bits(rng, base, 8 * j)
        d = np.linalg.norm(Xw - Ow)
        nrm = (Xw - Ow) / d
        n = len(mem)
        flags = np.full(n, synth.MP_HAS_OBS, np.uint8)
        if no_obs_every:
            flags[1::no_obs_every] = 0
        one = {"Xw": np.tile(Xw, (n, 1)).astype(np.float32), "normal": np.tile(nrm, (n, 1)).astype(np.float32),
               "max_dist": np.full(n, 1.2 * 0.999 * d, np.float32), "min_dist": np.full(n, 0.3 * d, np.float32),
               "desc": np.tile(base, (n, 1)), "flags": flags}
        if mp is None:
            mp = one
        else:
            for k, v in one.items():
                mp[k][mem] = v
    fr = dict(fr, keys_un=kp, desc=desc, u_right=np.full(len(kp), -1, np.float32))
    # frame-to-frame: the last frame sees every map point once, same octave 0, angles equal
    nl = n_total
    lk = np.zeros(nl, kp.dtype)
    lk["octave"] = 0
    lk["angle"] = kp["angle"][0]
    last = dict(p["last"], keys_un=lk, u_right=np.full(nl, -1, np.float32), desc=np.zeros((nl, 32), np.uint8))
    out = dict(p, frame=fr, map=mp, last=last, last_mp=np.arange(nl, dtype=np.int32),
               last_outlier=np.zeros(nl, np.uint8), kp_blocked=None)
    out["crowd"] = {"members": members, "n_near": n_kp_near}
    return out


def crowd_expected_owner(p, gate: int = 100, every_claim_blocks: bool = False):
    """The sequential rule on a crowd, by construction: each member in query order takes its crowd's
    unblocked keypoint with the fewest flipped bits (distance 8 * j) if that is <= gate; the keypoint is
    blocked for later members if the member has observations (or always, in the relocalisation / Sim3
    searches). Returns {keypoint index: owning map point} for the crowds' keypoints."""
    cr = p["crowd"]
    flags = p["map"]["flags"]
    order = sorted((q, c) for c, mem in enumerate(cr["members"]) for q in mem)
    blocked = [set() for _ in cr["members"]]
    owner = {}
    for q, c in order:
        free = [j for j in range(cr["n_near"]) if j not in blocked[c]]
        if not free or 8 * free[0] > gate:
            continue
        j = free[0]
        owner[c * cr["n_near"] + j] = q
        if every_claim_blocks or (flags[q] & synth.MP_HAS_OBS):
            blocked[c].add(j)
    return owner


def crowd_window_replay(p, want: int, gate: int = 100, every_claim_blocks: bool = False):
    """The resolve kernels' schedule on a crowd problem, restated: 64 queries are decided at once against the
    claims as of the window start, each from its kept four best candidates (a member's are keypoints 0..3 of
    its crowd), taking the first `want` unblocked ones (2 in track_local_resolve_kernel: best and second; 1
    in track_frame_resolve_kernel). A member with fewer than `want` left is a fallback, a member that
    examined a keypoint an earlier lane of the window claims is a conflict; the window is cut at the first of
    either, a fallback is rescanned over all its keypoints, a conflict restarts the window at its lane.
    Ordinary points have no candidates here (the CPU test shows it) and never stop a window.
    Returns (owners {keypoint: map point}, stops [(query, lane, "fallback" | "conflict")])."""
    cr = p["crowd"]
    n_near, flags, n_q = cr["n_near"], p["map"]["flags"], len(p["map"]["Xw"])
    crowd_of = {q: c for c, mem in enumerate(cr["members"]) for q in mem}
    blocks = lambda q: every_claim_blocks or bool(flags[q] & synth.MP_HAS_OBS)   # noqa: E731
    kept = min(4, n_near)
    claimed, owner, stops, base = set(), {}, [], 0
    while base < n_q:
        tag, lanes = {}, []
        for lane in range(min(64, n_q - base)):
            q = base + lane
            if q not in crowd_of:
                lanes.append(None)
                continue
            k0 = crowd_of[q] * n_near
            found, examined = [], []
            for j in range(kept):
                examined.append(k0 + j)
                if k0 + j not in claimed:
                    found.append(j)
                    if len(found) == want:
                        break
            fallback = n_near > 4 and len(found) < want
            accept = bool(found) and not fallback and 8 * found[0] <= gate
            if accept and blocks(q):
                tag[k0 + found[0]] = min(tag.get(k0 + found[0], 64), lane)
            lanes.append((q, k0, found, examined, fallback, accept))
        cut, kind = 64, None
        for lane, d in enumerate(lanes):
            if d is None:
                continue
            conflict = any(tag.get(k, 64) < lane for k in d[3])
            if conflict or d[4]:
                cut, kind = lane, "fallback" if d[4] else "conflict"
                break
        for lane, d in enumerate(lanes[:cut]):
            if d is not None and d[5]:
                q, k0, found = d[0], d[1], d[2]
                owner[k0 + found[0]] = max(owner.get(k0 + found[0], -1), q) if want == 2 else q
                if blocks(q):
                    claimed.add(k0 + found[0])
        if kind is None:
            base += 64
            continue
        q, k0 = lanes[cut][0], lanes[cut][1]
        stops.append((q, cut, kind))
        if kind == "fallback":
            free = [j for j in range(n_near) if k0 + j not in claimed]
            if free and 8 * free[0] <= gate:
                owner[k0 + free[0]] = q
                if blocks(q):
                    claimed.add(k0 + free[0])
            base += cut + 1
        else:
            base += cut
    return owner, stops
