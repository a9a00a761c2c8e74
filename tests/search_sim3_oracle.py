"""A numpy restatement of ORBmatcher::SearchBySim3 (reference src/ORBmatcher.cc:1102-1326 with KeyFrame::GetFeaturesInArea /
IsInImage, KeyFrame.cc:570-614, MapPoint::PredictScale, MapPoint.cc:391-406, and Frame::PosInGrid, Frame.cc:419-429), the yardstick
of qsp_search_by_sim3_batch, plus the fixtures its tests share.  Written here from the formulas.

Two flavours:
  "f32"  the reference's float32 operations in its order: cv::Mat products of small matrices are row sums in double rounded to
         float32 once with t added in float32, (1.0 / s12) * R12.t() is one double factor rounded to float32, 1.0 / z and cv::norm
         work in double and are rounded once, u = fx * x + cx is a float32 multiply and a float32 add, logf;
  "f64"  the same geometry in float64 from the float32 inputs.
The frame's own grid (which cell a key point was filed under, PosInGrid in float32) is data of the frame and the same in both;
descriptor distances and the tie-break are integer and the same in both.  Two traversals: "grid" walks a real mGrid as
GetFeaturesInArea does (ix outside iy, cell lists in index order, `dist < bestDist`); "brute" visits every key point and keeps the
minimum of the key dist << 40 | cell x << 33 | cell y << 26 | index -- the form of csrc/search_sim3.hpp.

Per source slot the restatement also returns the KNIFE-EDGE DISTANCE: the smallest relative distance of any decision to its
threshold -- |z| / dist3D against 0; u, v against the four bounds (relative to the image's extent); dist3D against both limits
(relative to the limit); log(ratio) / log_scale against the integers at which the clamped level changes (in levels); and for every
filed target key point ||dx| - r| / r, ||dy| - r| / r and the distance of the visited range's unrounded ends to the values at which
the key point's cell enters or leaves the range (in cells).  Slots without a point or with `pre` set decide nothing: inf."""
import functools
import os

import numpy as np

f32, f64 = np.float32, np.float64
TH_HIGH = 100
TH = 7.5
NO_POINT, PRE, Z_NEG, OUTSIDE, NEAR, FAR, EMPTY, SEARCHED = range(8)           # what became of a source slot
REASONS = ("no_point", "pre", "z_neg", "outside", "near", "far", "empty", "searched")


def _rowdot(R, X, F):
    """R (3,3) times X (3,) the way OpenCV's small-matrix product leaves it: each row summed in double, rounded to F once"""
    r, x = R.astype(f64), X.astype(f64)
    return ((r[:, 0] * x[0] + r[:, 1] * x[1]) + r[:, 2] * x[2]).astype(F)


def _round_half_away(v):
    """C's round() on float32 values, exactly (numpy's rounds half to even)"""
    v = v.astype(f64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def cells(frame):
    """Frame::PosInGrid for every key point: cell x, cell y and whether the key point was filed at all"""
    kp = np.asarray(frame["kp"], f32).reshape(-1, 2)
    min_x, _, min_y, _ = [f32(b) for b in frame["bounds"]]
    cols, rows, w_inv, h_inv = int(frame["grid"][0]), int(frame["grid"][1]), f32(frame["grid"][2]), f32(frame["grid"][3])
    cx = _round_half_away((kp[:, 0] - min_x) * w_inv)
    cy = _round_half_away((kp[:, 1] - min_y) * h_inv)
    return cx, cy, (cx >= 0) & (cx < cols) & (cy >= 0) & (cy < rows)


def build_grid(frame):
    """mGrid[ix][iy]: the indices filed under each cell, in index order (Frame::AssignFeaturesToGrid)"""
    cx, cy, ok = cells(frame)
    grid = [[[] for _ in range(int(frame["grid"][1]))] for _ in range(int(frame["grid"][0]))]
    for j in np.nonzero(ok)[0]:
        grid[cx[j]][cy[j]].append(int(j))
    return grid


def popcount_rows(a, b):
    """Hamming distance of the 256-bit rows a (n,32) to the row b (32,)"""
    return np.unpackbits(np.bitwise_xor(a, b[None, :]), axis=1).sum(1).astype(np.int64)


def transforms(cand, F):
    """(sR21, t21) for direction 0 and (sR12, t12) for direction 1, :1119-1121"""
    s, R, t = f32(cand["s12"]), np.asarray(cand["R12"], f32).reshape(3, 3), np.asarray(cand["t12"], f32).reshape(3)
    if F is f32:
        sR21 = ((1.0 / f64(s)) * R.T.astype(f64)).astype(f32)
        return (sR21, -_rowdot(sR21, t, f32)), (s * R, t)
    s, R, t = f64(s), R.astype(f64), t.astype(f64)
    sR21 = (1.0 / s) * R.T
    t21 = -((sR21[:, 0] * t[0] + sR21[:, 1] * t[1]) + sR21[:, 2] * t[2])
    return (sR21, t21), (s * R, t)


def _target(frame):
    cx, cy, ok = cells(frame)
    return dict(cx=cx, cy=cy, ok=ok, grid=build_grid(frame), kp=np.asarray(frame["kp"], f32).reshape(-1, 2),
                octave=np.asarray(frame["octave"], np.int64).reshape(-1), desc=np.asarray(frame["desc"], np.uint8).reshape(-1, 32))


MUTANTS = ("src_pyramid", "cand0_K", "cand0_th", "swap_rows_cols", "no_lower_clamp", "no_upper_clamp", "gate_unclamped")


def one_pass(S, T, cand, direction, pre, flavour, traversal="grid", tgt=None, mutant=None, first=None):
    """One direction of SearchBySim3 over the source frame S into the target frame T.  Returns dict(best, dist (n,) int64 with dist
    -1 where no key point was eligible, knife (n,), reason (n,) and info: one dict per searched slot with what the tests count).
    `mutant` (brute traversal only) makes ONE of the mistakes a kernel or a staging loop could make, so that the tests can show
    which fixtures notice it: the SOURCE's pyramid (log_scale, n_levels, scale factors) for PredictScale; K or th of `first`, the
    batch's candidate 0; the target's grid_rows and grid_cols swapped; PredictScale without its lower or its upper clamp (scale
    factors continued geometrically); the octave gate evaluated with the unclamped level.  The knife-edge distances are the true ones."""
    assert mutant is None or (mutant in MUTANTS and traversal == "brute")
    F = f32 if flavour == "f32" else f64
    tgt = tgt or _target(T)
    n = int(np.size(S["octave"]))
    M, t = transforms(cand, F)[direction]
    K = np.asarray((first if mutant == "cand0_K" else cand)["K"], f32).astype(F)
    th = F(f32((first if mutant == "cand0_th" else cand).get("th", TH)))
    Rcw, tcw = np.asarray(S["Rcw"], f32).reshape(3, 3), np.asarray(S["tcw"], f32).reshape(3)
    min_x, max_x, min_y, max_y = [F(f32(b)) for b in T["bounds"]]
    cols, rows, w_inv, h_inv = int(T["grid"][0]), int(T["grid"][1]), F(f32(T["grid"][2])), F(f32(T["grid"][3]))
    P = S if mutant == "src_pyramid" else T
    sf, n_levels, log_scale = np.asarray(P["scale_factors"], f32).astype(F), int(np.size(P["scale_factors"])), F(f32(P["log_scale"]))
    filed = tgt["ok"]
    if mutant == "swap_rows_cols":
        cols, rows = rows, cols
        filed = (tgt["cx"] >= 0) & (tgt["cx"] < cols) & (tgt["cy"] >= 0) & (tgt["cy"] < rows)
    kx, ky = tgt["kp"][:, 0].astype(F), tgt["kp"][:, 1].astype(F)
    best, dist = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    knife, reason, info = np.full(n, np.inf), np.zeros(n, np.int64), {}
    for i in range(n):
        if not S["has_point"][i]:
            reason[i] = NO_POINT
            continue
        if pre[i]:
            reason[i] = PRE
            continue
        Xw = np.asarray(S["Xw"], f32).reshape(-1, 3)[i]
        with np.errstate(all="ignore"):
            if F is f32:
                pc = _rowdot(Rcw, Xw, f32) + tcw
                p = _rowdot(M, pc, f32) + t
                invz = f32(1.0 / f64(p[2]))
                d3 = f32(np.sqrt((f64(p[0]) * f64(p[0]) + f64(p[1]) * f64(p[1])) + f64(p[2]) * f64(p[2])))
            else:
                R, X = Rcw.astype(f64), Xw.astype(f64)
                pc = ((R[:, 0] * X[0] + R[:, 1] * X[1]) + R[:, 2] * X[2]) + tcw.astype(f64)
                p = ((M[:, 0] * pc[0] + M[:, 1] * pc[1]) + M[:, 2] * pc[2]) + t
                invz = 1.0 / p[2]
                d3 = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
            k = [abs(float(p[2])) / float(d3)]
            if p[2] < 0:
                reason[i], knife[i] = Z_NEG, k[0]
                continue
            x, y = p[0] * invz, p[1] * invz
            u, v = K[0] * x + K[2], K[1] * y + K[3]
            k += [abs(float(u - b)) / float(max_x - min_x) for b in (min_x, max_x)] + [abs(float(v - b)) / float(max_y - min_y) for b in (min_y, max_y)]
            if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
                reason[i], knife[i] = OUTSIDE, min(k)
                continue
            dmin, dmaxi = F(f32(S["dist_min_inv"][i])), F(f32(S["dist_max_inv"][i]))
            k += [abs(float(d3 - dmin)) / float(dmin), abs(float(d3 - dmaxi)) / float(dmaxi)]
            if d3 < dmin or d3 > dmaxi:
                reason[i], knife[i] = (NEAR if d3 < dmin else FAR), min(k)
                continue
            ratio = F(f32(S["dist_max"][i])) / d3
            q = np.log(ratio) / log_scale                         # (numpy's float32 log stands in for logf)
            k += [abs(float(q) - e) for e in range(n_levels - 1)]  # ceil(q) clamped to [0, n_levels - 1] changes at 0 .. n_levels - 2
            level = gate = int(min(max(np.ceil(q), 0), n_levels - 1))
            if mutant == "no_lower_clamp":
                level = gate = int(min(np.ceil(q), n_levels - 1))
            elif mutant == "no_upper_clamp":
                level = gate = int(max(np.ceil(q), 0))
            elif mutant == "gate_unclamped":
                gate = int(np.ceil(q))
            r = th * (sf[level] if 0 <= level < n_levels else F(np.exp(f64(log_scale)) ** level))
            a_x, b_x, a_y, b_y = ((u - min_x) - r) * w_inv, ((u - min_x) + r) * w_inv, ((v - min_y) - r) * h_inv, ((v - min_y) + r) * h_inv
            lo_x, hi_x, lo_y, hi_y = int(np.floor(a_x)), int(np.ceil(b_x)), int(np.floor(a_y)), int(np.ceil(b_y))
            min_cx, max_cx, min_cy, max_cy = max(0, lo_x), min(cols - 1, hi_x), max(0, lo_y), min(rows - 1, hi_y)
            dx, dy = np.abs(kx - u), np.abs(ky - v)
            ok = tgt["ok"]
            if ok.any():
                cx, cy = tgt["cx"][ok].astype(f64), tgt["cy"][ok].astype(f64)
                k += [float(np.min(np.abs(dx[ok] - r) / r)), float(np.min(np.abs(dy[ok] - r) / r)),
                      float(np.min(np.abs(f64(a_x) - (cx + 1)))), float(np.min(np.abs(f64(b_x) - (cx - 1)))),
                      float(np.min(np.abs(f64(a_y) - (cy + 1)))), float(np.min(np.abs(f64(b_y) - (cy - 1))))]
        knife[i] = min(k)
        in_box = (dx < r) & (dy < r)
        if traversal == "grid":
            found = []
            if not (min_cx >= cols or max_cx < 0 or min_cy >= rows or max_cy < 0):
                for ix in range(min_cx, max_cx + 1):
                    for iy in range(min_cy, max_cy + 1):
                        found += [j for j in tgt["grid"][ix][iy] if in_box[j]]
            found = np.array(found, np.int64)
        else:
            elig = filed & (tgt["cx"] >= min_cx) & (tgt["cx"] <= max_cx) & (tgt["cy"] >= min_cy) & (tgt["cy"] <= max_cy) & in_box
            found = np.nonzero(elig)[0]
        octs = tgt["octave"][found]
        keep = found[(octs >= gate - 1) & (octs <= gate)]
        inf = dict(level=level, q=float(q), lo_x=lo_x, hi_x=hi_x, lo_y=lo_y, hi_y=hi_y, octaves=sorted(set(int(o) - level for o in octs)),
                   tie=False, tie_same_cx=False, unfiled_in_box=int((in_box & ~ok).sum()))
        info[i] = inf
        if len(found) == 0:
            reason[i] = EMPTY
            continue
        reason[i] = SEARCHED
        if len(keep) == 0:
            continue
        hd = popcount_rows(tgt["desc"][keep], np.asarray(S["mp_desc"], np.uint8).reshape(-1, 32)[i])
        if traversal == "grid":
            b, bd = -1, 1 << 30
            for j, d in zip(keep, hd):                          # `dist < bestDist`: the first of the traversal stays
                if d < bd:
                    b, bd = int(j), int(d)
        else:
            key = (hd << 40) | (tgt["cx"][keep] << 33) | (tgt["cy"][keep] << 26) | keep
            kmin = int(key.min())
            b, bd = kmin & ((1 << 26) - 1), kmin >> 40
        dist[i] = bd
        if bd <= TH_HIGH:
            best[i] = b
        ties = keep[hd == bd]
        if len(ties) > 1 and int(ties.min()) != b:              # the lowest index is not the traversal's first
            inf["tie"] = True
            inf["tie_same_cx"] = bool(tgt["cx"][int(ties.min())] == tgt["cx"][b])
    return dict(best=best, dist=dist, knife=knife, reason=reason, info=info)


def search(kf1, cand, flavour, traversal="grid", tgt1=None, mutant=None, first=None):
    """SearchBySim3 of one candidate: both passes, the agreement step (:1307-1323) and the knife-edge distances"""
    kf2 = cand["kf2"]
    n1, n2 = int(np.size(kf1["octave"])), int(np.size(kf2["octave"]))
    pre1 = np.zeros(n1, np.uint8) if cand.get("pre1") is None else np.asarray(cand["pre1"], np.uint8)
    pre2 = np.zeros(n2, np.uint8) if cand.get("pre2") is None else np.asarray(cand["pre2"], np.uint8)
    a = one_pass(kf1, kf2, cand, 0, pre1, flavour, traversal, mutant=mutant, first=first)
    b = one_pass(kf2, kf1, cand, 1, pre2, flavour, traversal, tgt=tgt1, mutant=mutant, first=first)
    match = np.full(n1, -1, np.int64)
    for i1 in range(n1):
        j = a["best"][i1]
        if j >= 0 and b["best"][j] == i1:
            match[i1] = j
    return dict(best1=a["best"], dist1=a["dist"], best2=b["best"], dist2=b["dist"], match12=match, n_found=int((match >= 0).sum()),
                knife1=a["knife"], knife2=b["knife"], reason1=a["reason"], reason2=b["reason"], info1=a["info"], info2=b["info"])


# ---- fixtures -----------------------------------------------------------------------------------------------------------
N1, N_COMMON = 130, 100
N_LEVELS, SCALE = 8, f32(1.2)
SF = np.array([SCALE ** i for i in range(N_LEVELS)], f32)
LOG_SCALE = f32(np.log(SCALE))
CAM = np.array([517.3, 516.5, 318.6, 255.3], f32)              # key frame 1's fx fy cx cy: used for both directions
BOUNDS_VGA, GRID_VGA = (0.0, 640.0, 0.0, 480.0), (64, 48, f32(64) / f32(640), f32(48) / f32(480))
BOUNDS_SMALL, GRID_SMALL = (0.0, 128.0, 0.0, 96.0), (64, 48, f32(64) / f32(128), f32(48) / f32(96))


def _rot(rng, angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _pix(Y):
    return np.stack([CAM[0] * Y[..., 0] / Y[..., 2] + CAM[2], CAM[1] * Y[..., 1] / Y[..., 2] + CAM[3]], -1)


def _unpix(uv, z):
    return np.array([(uv[0] - CAM[2]) / CAM[0] * z, (uv[1] - CAM[3]) / CAM[1] * z, z])


def _flip(rng, d, nbits):
    """a copy of the 32-byte descriptor d with nbits different bits flipped"""
    bits = np.unpackbits(d)
    idx = rng.choice(256, nbits, replace=False)
    bits[idx] ^= 1
    return np.packbits(bits)


def _mp_fields(n):
    return dict(has_point=np.ones(n, np.uint8), Xw=np.zeros((n, 3), f32), dist_min_inv=np.zeros(n, f32), dist_max_inv=np.zeros(n, f32),
                dist_max=np.zeros(n, f32), mp_desc=np.zeros((n, 32), np.uint8))


def _set_point(fr, i, Yc, level, desc, Rcw, tcw, q_off=-0.5):
    """slot i of frame fr gets a map point at camera coordinates Yc (of that frame) whose predicted level, seen from about that
    distance, is `level` (log(ratio) / log_scale = level + q_off) and the ordinary invariance limits"""
    fr["Xw"][i] = (Rcw.T @ (Yc - tcw)).astype(f32)
    d = float(np.linalg.norm(Yc))
    fr["dist_max"][i] = f32(d * float(SCALE) ** (level + q_off))
    fr["dist_max_inv"][i] = f32(1.2) * fr["dist_max"][i]
    fr["dist_min_inv"][i] = f32(0.8) * f32(fr["dist_max"][i] / SF[-1])
    fr["mp_desc"][i] = desc


# slots of key frame 1 beyond the common points
S_NOPOINT, S_BEHIND, S_OUT_U, S_OUT_V, S_NEAR, S_FAR, S_CLAMP0, S_CLAMPTOP = 100, 102, 104, 105, 106, 107, 108, 110
S_CORNER = (112, 113, 114, 115, 116, 117)                      # project into the top-left 128 x 96 pixels
CORNER_UV = ((3.4, 4.3), (124.6, 92.7), (60.2, 50.9), (3.7, 91.6), (125.3, 3.2), (70.8, 20.1))
S_SPECIAL = tuple(range(118, 130))                             # sources of the hand-made cases of special_candidate
SPECIAL_UV = [(150.3 + 37.1 * k, 120.2 + 23.3 * (k % 5)) for k in range(12)]
SPECIAL_LEVEL = 2
SEED_SPECIAL = 77


@functools.lru_cache(maxsize=None)
def world():
    """what all fixtures share: key frame 1's pose, the common points in its camera frame with their descriptors and levels"""
    rng = np.random.default_rng(20261)
    R1, t1 = _rot(rng, 0.4), rng.normal(size=3) * 0.5
    uv = np.stack([rng.uniform(140, 600, N1), rng.uniform(110, 440, N1)], -1)
    for s, p in zip(S_CORNER, CORNER_UV):
        uv[s] = p
    for s, p in zip(S_SPECIAL, SPECIAL_UV):
        uv[s] = p
    z = rng.uniform(3.0, 8.0, N1)
    z[list(S_SPECIAL)] = 5.0
    Y = np.stack([_unpix(uv[i], z[i]) for i in range(N1)])
    s12, R12, t12 = _sim3(SEED_SPECIAL)[:3]                      # slot 123 projects to the right edge of the special candidate's frame
    Y[NAMED["unfiled"]] = s12 * (R12 @ _unpix((631.0, 200.0), 5.0)) + t12
    Y[S_BEHIND], Y[S_BEHIND + 1] = (0.3, 0.2, -3.0), (-0.4, 0.1, -5.0)
    Y[S_OUT_U], Y[S_OUT_V] = _unpix((-300.0, 200.0), 4.0), _unpix((300.0, 900.0), 4.0)
    desc = rng.integers(0, 256, (N1, 32)).astype(np.uint8)
    level = rng.integers(1, N_LEVELS - 1, N1)
    level[list(S_SPECIAL)] = SPECIAL_LEVEL
    return dict(R1=R1.astype(f32), t1=t1.astype(f32), Y=Y, desc=desc, level=level)


@functools.lru_cache(maxsize=None)
def key_frame_1():
    """the current key frame: 130 slots; treat as read-only"""
    w = world()
    rng = np.random.default_rng(20262)
    R1, t1 = w["R1"].astype(f64), w["t1"].astype(f64)
    fr = dict(bounds=BOUNDS_VGA, grid=GRID_VGA, log_scale=LOG_SCALE, scale_factors=SF.copy(), Rcw=w["R1"], tcw=w["t1"], **_mp_fields(N1))
    kp = np.zeros((N1, 2), f32)
    octave = np.zeros(N1, np.int32)
    desc = np.zeros((N1, 32), np.uint8)
    for i in range(N1):
        Y = w["Y"][i]
        _set_point(fr, i, Y, int(w["level"][i]), _flip(rng, w["desc"][i], int(rng.integers(0, 12))), R1, t1)
        kp[i] = _pix(Y if Y[2] > 0 else np.array([0.1 * i, 0.2, 4.0])) + rng.normal(size=2) * 0.7
        octave[i] = int(w["level"][i]) - int(rng.integers(0, 2))
        desc[i] = _flip(rng, w["desc"][i], int(rng.integers(0, 12)))
    kp[S_OUT_U], kp[S_OUT_V] = (20.5, 30.5), (620.5, 470.5)
    fr["has_point"][[S_NOPOINT, S_NOPOINT + 1]] = 0
    fr["dist_min_inv"][S_NEAR] = f32(50.0)                                          # nearer than the lower limit
    fr["dist_max_inv"][S_FAR] = f32(0.5)                                            # farther than the upper limit
    for s, q in ((S_CLAMP0, -2.6), (S_CLAMP0 + 1, -0.4), (S_CLAMPTOP, 9.3), (S_CLAMPTOP + 1, 7.6)):
        fr["dist_max"][s] = f32(np.linalg.norm(w["Y"][s]) * float(SCALE) ** q)      # log(ratio) / log_scale is about q from any near view
        fr["dist_min_inv"][s], fr["dist_max_inv"][s] = f32(0.01), f32(1000.0)
    fr.update(kp=kp, octave=octave, desc=desc)
    return fr


@functools.lru_cache(maxsize=None)
def target_1():
    return _target(key_frame_1())


def _sim3(seed):
    rng = np.random.default_rng(9000 + seed)
    return float(rng.uniform(0.85, 1.2)), _rot(rng, 0.15), rng.normal(size=3) * 0.25, _rot(rng, 0.5), rng.normal(size=3) * 0.6


def _to_cam2(s12, R12, t12, Y1):
    return (1.0 / s12) * (R12.T @ (Y1 - t12))


def make_candidate(seed, n2, small=False, kind="planted"):
    """kind 'planted': slot j < min(n2, 100) of key frame 2 holds common point perm[j], seen about a pixel off; later slots are
    unrelated key points, every third without a map point.  'no_points': the same frame with no map point in any slot.
    'all_pre1': pre1 set on every slot.  small: a 128 x 96 image on the 64 x 48 grid; its common points are the corner slots."""
    w, k1 = world(), key_frame_1()
    rng = np.random.default_rng(31000 + 100 * seed + n2)
    s12, R12, t12, R2, t2 = _sim3(seed)
    if small:
        s12, R12, t12 = 1.0 + 0.01 * seed, _rot(rng, 0.004), rng.normal(size=3) * 0.004
    fr = dict(bounds=BOUNDS_SMALL if small else BOUNDS_VGA, grid=GRID_SMALL if small else GRID_VGA, log_scale=LOG_SCALE,
              scale_factors=SF.copy(), Rcw=R2.astype(f32), tcw=t2.astype(f32), **_mp_fields(n2))
    R2, t2 = fr["Rcw"].astype(f64), fr["tcw"].astype(f64)
    kp, octave, desc = np.zeros((n2, 2), f32), np.zeros(n2, np.int32), np.zeros((n2, 32), np.uint8)
    src = list(S_CORNER) + list(rng.permutation(N_COMMON)) if small else list(rng.permutation(N_COMMON))
    lo, hi = np.array(fr["bounds"])[[0, 2]], np.array(fr["bounds"])[[1, 3]]
    for j in range(n2):
        if j < len(src):
            i1 = int(src[j])
            Z = _to_cam2(s12, R12, t12, w["Y"][i1]) + rng.normal(size=3) * 0.003
            lvl = int(w["level"][i1])
            _set_point(fr, j, Z, lvl, _flip(rng, w["desc"][i1], int(rng.integers(0, 12))), R2, t2)
            kp[j] = _pix(Z) + rng.normal(size=2) * 0.7
            octave[j] = lvl - int(rng.integers(0, 2))
            desc[j] = _flip(rng, w["desc"][i1], int(rng.integers(0, 12)))
        else:
            uv = rng.uniform(lo + 1, hi - 1)
            Z = _unpix(uv + rng.normal(size=2) * 3, rng.uniform(3.0, 8.0))
            lvl = int(rng.integers(1, N_LEVELS - 1))
            _set_point(fr, j, Z, lvl, rng.integers(0, 256, 32).astype(np.uint8), R2, t2)
            kp[j], octave[j], desc[j] = uv, lvl, rng.integers(0, 256, 32).astype(np.uint8)
            fr["has_point"][j] = j % 3 != 0
    if small and n2:
        kp[min(n2, 40) - 1] = (127.3, 95.2)                    # round(127.3 / 2) == 64 == grid_cols: never filed
    if kind == "no_points":
        fr["has_point"][:] = 0
    fr.update(kp=kp, octave=octave, desc=desc)
    pre1, pre2 = np.zeros(N1, np.uint8), np.zeros(n2, np.uint8)
    if kind == "all_pre1":
        pre1[:] = 1
    elif n2 > 8:                                               # an earlier match: slot 5 of key frame 1 with slot 3 of key frame 2
        pre1[5], pre2[3] = 1, 1
        pre1[9] = 1                                            # ... and one whose point has no index in key frame 2
    return dict(kf2=fr, K=CAM.copy(), s12=f32(s12), R12=R12.astype(f32), t12=t12.astype(f32), th=f32(TH), pre1=pre1, pre2=pre2,
                kind=kind, small=small)


# the hand-made cases: name -> the slot of key frame 1 that is their source
NAMED = dict(tie_cx=118, tie_cy=119, tie_cx_far=120, th_100=121, th_101=122, unfiled=123, octaves=124, no_mutual=125, pre2_best=126,
             empty_box=127)


@functools.lru_cache(maxsize=None)
def special_candidate():
    """Key frame 2 built around the projections of key frame 1's slots 118..129 (level 2: radius 7.5 * 1.44 = 10.8 pixels; octaves 1
    and 2 pass).  Every case sits in its own box, the boxes are 37 pixels apart.  Offsets are from the float64 projection."""
    w, k1 = world(), key_frame_1()
    rng = np.random.default_rng(4242)
    s12, R12, t12, R2, t2 = _sim3(SEED_SPECIAL)
    R2, t2 = R2.astype(f32).astype(f64), t2.astype(f32).astype(f64)
    rows = []                                                  # (kp, octave, desc, map point or None)
    L = SPECIAL_LEVEL

    def centre(i1):
        return _pix(_to_cam2(s12, R12, t12, w["Y"][i1]))

    def add(uv, octave, desc, point=None):
        rows.append((np.asarray(uv, f64), octave, desc, point))
        return len(rows) - 1

    def own_point(i1, desc):
        """a map point at the place of key frame 1's slot i1, so that the pass back lands on that slot's key point"""
        return dict(Z=_to_cam2(s12, R12, t12, w["Y"][i1]), desc=desc, level=int(w["level"][i1]), i1=i1)

    junk = lambda: rng.integers(0, 256, 32).astype(np.uint8)
    d = {k: k1["mp_desc"][i] for k, i in NAMED.items()}        # the source map points' descriptors
    # ties: two key points at the same distance; the LOWER index lies later in (cell x, cell y, index) order
    c = centre(NAMED["tie_cx"])
    add(c + (6.1, -3.2), L, _flip(rng, d["tie_cx"], 7))        # index 0: cell x larger
    add(c + (-6.3, 2.1), L, _flip(rng, d["tie_cx"], 7), own_point(NAMED["tie_cx"], k1["desc"][NAMED["tie_cx"]]))   # index 1: first in the walk
    c = centre(NAMED["tie_cy"])
    c = np.array([np.floor(c[0] / 10) * 10 + 2.0, c[1]])       # both in the same cell column: x' in [.., + 0.35]
    t0 = add(c + (0.4, 7.3), L - 1, _flip(rng, d["tie_cy"], 9))                 # index 2: same cell x, cell y larger
    add(c + (1.1, -7.1), L, _flip(rng, d["tie_cy"], 9))        # index 3: cell y smaller, the walk's first
    c = centre(NAMED["tie_cx_far"])
    add(c + (9.7, 9.2), L, _flip(rng, d["tie_cx_far"], 3))     # index 4
    add(c + (0.3, -0.4), L, _flip(rng, d["tie_cx_far"], 3))    # index 5
    add(c + (-9.9, 9.6), L - 1, _flip(rng, d["tie_cx_far"], 3))  # index 6: the smallest cell x wins over 4 and 5
    # TH_HIGH: a lone key point at distance exactly 100, and one at exactly 101
    add(centre(NAMED["th_100"]) + (1.2, 0.7), L, _flip(rng, d["th_100"], 100))
    add(centre(NAMED["th_101"]) + (-0.8, 1.1), L, _flip(rng, d["th_101"], 101))
    # a key point that was never filed (round(636.2 / 10) == 64 == grid_cols) with the perfect descriptor, next to a filed one at
    # distance 40; world() puts the source's projection at about (631, 200)
    c = centre(NAMED["unfiled"])
    uf = add(c + (-3.0, -1.0), L, _flip(rng, d["unfiled"], 40))
    add((636.2, c[1] + 1.0), L, d["unfiled"].copy())
    # octaves level - 2 .. level + 1 in one box: the perfect descriptors are at level - 2 and level + 1
    c = centre(NAMED["octaves"])
    add(c + (1.0, 1.0), L - 2, d["octaves"].copy())
    add(c + (-2.0, 1.5), L + 1, d["octaves"].copy())
    add(c + (3.0, -2.0), L - 1, _flip(rng, d["octaves"], 30))
    add(c + (-3.5, -2.5), L, _flip(rng, d["octaves"], 20))
    # no mutual agreement: the key point's own map point projects onto another slot of key frame 1
    add(centre(NAMED["no_mutual"]) + (0.5, 0.5), L, _flip(rng, d["no_mutual"], 5), own_point(3, k1["desc"][3]))
    # pre2 on the best key point: pass 1 -> 2 takes it all the same, pass 2 -> 1 skips it as a source
    pb = add(centre(NAMED["pre2_best"]) + (0.6, -0.4), L, _flip(rng, d["pre2_best"], 4), own_point(NAMED["pre2_best"], k1["desc"][NAMED["pre2_best"]]))
    # empty_box: nothing near slot 127's projection
    n2 = len(rows)
    fr = dict(bounds=BOUNDS_VGA, grid=GRID_VGA, log_scale=LOG_SCALE, scale_factors=SF.copy(), Rcw=R2.astype(f32), tcw=t2.astype(f32), **_mp_fields(n2))
    kp, octave, desc = np.zeros((n2, 2), f32), np.zeros(n2, np.int32), np.zeros((n2, 32), np.uint8)
    for j, (uv, o, de, pt) in enumerate(rows):
        kp[j], octave[j], desc[j] = uv, o, de
        if pt is None:
            fr["has_point"][j] = 0
        else:
            _set_point(fr, j, pt["Z"], pt["level"], pt["desc"], R2, t2)
            # seen from key frame 1 (the scale changes the distance) the predicted level is that key point's octave + 1
            fr["dist_max"][j] = f32(np.linalg.norm(w["Y"][pt["i1"]]) * float(SCALE) ** (int(k1["octave"][pt["i1"]]) + 0.5))
            fr["dist_max_inv"][j], fr["dist_min_inv"][j] = f32(1.2) * fr["dist_max"][j], f32(0.8) * f32(fr["dist_max"][j] / SF[-1])
    fr.update(kp=kp, octave=octave, desc=desc)
    pre1, pre2 = np.ones(N1, np.uint8), np.zeros(n2, np.uint8)
    pre1[list(NAMED.values())] = 0                             # only the named slots search: nothing else reaches into the boxes
    pre2[pb] = 1
    return dict(kf2=fr, K=CAM.copy(), s12=f32(s12), R12=R12.astype(f32), t12=t12.astype(f32), th=f32(TH), pre1=pre1, pre2=pre2,
                kind="special", small=False, pre2_best=pb, unfiled_filed=uf, tie_first=dict(tie_cx=1, tie_cy=3, tie_cx_far=6), tie_lowest=dict(tie_cx=0, tie_cy=t0, tie_cx_far=4))


# (n2, kind, small, seed): the wave-stride edges of the target loop (63, 64, 65, a third pass at 129, 300), an empty and a one-point
# target, a frame without map points, every pre1 set, the small image, the hand-made cases
POOL = [(0, "planted", False, 1), (1, "planted", False, 1), (63, "planted", False, 1), (64, "planted", False, 1), (65, "planted", False, 1),
        (129, "planted", False, 1), (300, "planted", False, 1), (65, "no_points", False, 2), (64, "all_pre1", False, 2),
        (40, "planted", True, 1), "special"]
I_SPECIAL, I_SMALL = 10, 9


@functools.lru_cache(maxsize=None)
def pool():
    """the candidates (inputs only; treat as read-only); all share key_frame_1()"""
    return [special_candidate() if p == "special" else make_candidate(p[3], p[0], small=p[2], kind=p[1]) for p in POOL]


@functools.lru_cache(maxsize=None)
def pool_results(flavour, traversal="grid"):
    return [search(key_frame_1(), c, flavour, traversal, tgt1=target_1()) for c in pool()]


def disagreements(a, b):
    """per direction: the source slots on which two results differ in best or dist"""
    return [(a["best%d" % d] != b["best%d" % d]) | (a["dist%d" % d] != b["dist%d" % d]) for d in (1, 2)]


@functools.lru_cache(maxsize=None)
def measured():
    """CPU: the largest knife-edge distance of a source slot on which the two flavours disagree, over the pool"""
    worst = 0.0
    for a, b in zip(pool_results("f32"), pool_results("f64")):
        for d, diff in zip((1, 2), disagreements(a, b)):
            if diff.any():
                worst = max(worst, float(b["knife%d" % d][diff].max()))
    return worst


def band():
    """what tests/test_gpu_search_sim3.py leaves undecided: 4 x the measured band"""
    return 4 * measured()


IN_BAND_CAP = 0.02                                             # at most this share of a candidate's source slots inside the band


def in_band_share(r64, width):
    k = np.concatenate([r64["knife1"], r64["knife2"]])
    return float((k < width).mean()) if k.size else 0.0


MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "search_sim3_margins.json")


# ---- the mixed pool: frames and candidates that differ from each other -----------------------------------------------------
# POOL's candidates share one pyramid, one camera, one th and one grid size, so an index mistake between source and target, or
# between candidate c and candidate 0, computes the same there.  Here everything a FrameP or a CandP carries differs between key
# frame 1 (key_frame_1(): 8 levels at 1.2, 640 x 480 on 64 x 48) and key frame 2, and from one candidate to the next.  The camera
# of a candidate is FITTED: of the 100 common points seen from key frame 2, the third smallest and third largest normalised
# coordinates land on `span` (u_lo, u_hi, v_lo, v_hi), so the cameras differ by hundreds of pixels, two points per side fall
# outside the image, and with span None the extreme ones sit in the first and last filed row and column of the grid
# (Frame::PosInGrid ROUNDS: the last half cell of an image is never filed, and of a 1 x 1 grid only the top-left quarter is).
POOL_MIXED = [
    dict(name="5 levels at 1.5", levels=5, scale=1.5, th=12.0, bounds=BOUNDS_VGA, grid=(64, 48), span=(60.0, 580.0, 50.0, 430.0), seed=21, s12=1.6),
    dict(name="16 levels at 1.1", levels=16, scale=1.1, th=5.0, bounds=BOUNDS_VGA, grid=(64, 48), span=(4.0, 630.0, 4.0, 470.0), seed=42),
    dict(name="1 level", levels=1, scale=1.2, th=7.5, bounds=BOUNDS_VGA, grid=(64, 48), span=(150.0, 490.0, 120.0, 360.0), seed=13),
    dict(name="8 levels at sqrt 2", levels=8, scale=float(np.sqrt(2.0)), th=5.0, bounds=BOUNDS_VGA, grid=(64, 48), span=(100.0, 560.0, 30.0, 450.0), seed=264),
    dict(name="1 x 1 grid", levels=8, scale=1.2, th=7.5, bounds=BOUNDS_VGA, grid=(1, 1), span=(2.0, 380.0, 2.0, 290.0), seed=15),
    dict(name="5 x 7 grid", levels=5, scale=1.5, th=12.0, bounds=(0.0, 320.0, 0.0, 240.0), grid=(5, 7), span=None, seed=16, s12=0.8),
    dict(name="64 x 64 grid", levels=16, scale=1.1, th=5.0, bounds=BOUNDS_VGA, grid=(64, 64), span=None, seed=27),
    dict(name="bounds off 0", levels=8, scale=float(np.sqrt(2.0)), th=7.5, bounds=(-12.5, 651.25, -8.25, 487.5), grid=(64, 48), span=None, seed=28),
]
THS = (5.0, 7.5, 12.0)
N2_MIXED = 128
S_GATES = (S_CLAMP0, S_CLAMP0 + 1, S_CLAMPTOP, S_CLAMPTOP + 1)  # sources of key frame 1 whose level is clamped in most pyramids
I_1X1 = 4


def _pixk(K, Y):
    return np.array([K[0] * Y[0] / Y[2] + K[2], K[1] * Y[1] / Y[2] + K[3]])


def _unpixk(K, uv, z):
    return np.array([(uv[0] - K[2]) / K[0] * z, (uv[1] - K[3]) / K[1] * z, z])


def _clamp_level(q, n_levels):
    return int(min(max(np.ceil(q), 0), n_levels - 1))


@functools.lru_cache(maxsize=None)
def make_mixed(index):
    """Candidate `index` of POOL_MIXED.  Slot j < 100 of key frame 2: a key point at the projection of common point perm[j] (octave: the
    level PredictScale gives with key frame 2's pyramid, or one below) and a map point that projects, with this candidate's camera,
    onto key frame 1's key point perm[j], with dist_max such that the level predicted with key frame 1's pyramid is that key
    point's octave or one above; where that octave is 0 or 6 every other such point gets log(ratio) / log_scale = -2.5 or 9.4, the
    two clamps of the pass 2 -> 1.  Then the hand-made key points (no map points) around the projections of sources of key frame 1,
    recorded under `named`; then unrelated key points up to N2_MIXED."""
    spec = POOL_MIXED[index]
    w, k1 = world(), key_frame_1()
    rng = np.random.default_rng(52000 + spec["seed"])
    r32 = lambda a: np.asarray(a, f32).astype(f64)
    s12, R12, t12, R2, t2 = _sim3(spec["seed"])
    s12, R12, t12, R2, t2 = float(f32(spec.get("s12", s12))), r32(R12), r32(t12), r32(R2), r32(t2)
    n_levels, scale, th = spec["levels"], f32(spec["scale"]), spec["th"]
    sf, log_scale = np.array([scale ** i for i in range(n_levels)], f32), f32(np.log(scale))
    min_x, max_x, min_y, max_y = spec["bounds"]
    cols, rows = spec["grid"]
    grid = (cols, rows, f32(cols) / f32(max_x - min_x), f32(rows) / f32(max_y - min_y))
    cw, ch = (max_x - min_x) / cols, (max_y - min_y) / rows
    span = spec["span"] or (min_x + 1.0, min_x + (cols - 0.9) * cw, min_y + 1.0, min_y + (rows - 0.9) * ch)
    Z = np.stack([_to_cam2(s12, R12, t12, w["Y"][i]) for i in range(N1)])      # key frame 1's points in key frame 2's camera
    assert (Z[:N_COMMON, 2] > 0).all()
    K = np.zeros(4)
    for a in (0, 1):
        xs = np.sort(Z[:N_COMMON, a] / Z[:N_COMMON, 2])
        K[a] = (span[2 * a + 1] - span[2 * a]) / (xs[-3] - xs[2])
        K[2 + a] = span[2 * a] - K[a] * xs[2]
    K = r32(K)
    c2 = np.stack([_pixk(K, z) for z in Z])
    q2 = np.log(k1["dist_max"].astype(f64) / np.linalg.norm(Z, axis=1)) / float(log_scale)
    L2 = [_clamp_level(q, n_levels) for q in q2]
    rows_, named = [], dict(gates={}, th_in=None, th_out=None, tie=None, clamp2_low=[], clamp2_top=[])

    def add(uv, octave, desc, point=None):
        rows_.append((np.asarray(uv, f64), int(octave), desc, point))
        return len(rows_) - 1

    for j, i1 in enumerate(rng.permutation(N_COMMON)):
        i1 = int(i1)
        Y1 = _unpixk(K, k1["kp"][i1].astype(f64) + rng.normal(size=2) * 0.5, w["Y"][i1][2])
        o1 = int(k1["octave"][i1])
        pt = dict(Z=_to_cam2(s12, R12, t12, Y1), d1=float(np.linalg.norm(Y1)), q=min(o1 + int(rng.integers(0, 2)), N_LEVELS - 1) - 0.5,
                  desc=_flip(rng, w["desc"][i1], int(rng.integers(0, 12))), wide=False)
        if o1 == 0 and len(named["clamp2_low"]) < 3:
            pt.update(q=-2.5, wide=True)
            named["clamp2_low"].append(j)
        elif o1 >= N_LEVELS - 2 and len(named["clamp2_top"]) < 3:
            pt.update(q=9.4, wide=True)
            named["clamp2_top"].append(j)
        add(c2[i1] + rng.normal(size=2) * 0.7, max(L2[i1] - int(rng.integers(0, 2)), 0), _flip(rng, w["desc"][i1], int(rng.integers(0, 12))), pt)

    def filed(uv):
        x, y = (uv[0] - min_x) / cw, (uv[1] - min_y) / ch
        return 0.0 < x < cols - 0.6 and 0.0 < y < rows - 0.6       # inside the image and short of the half cell that is never filed

    d = lambda s: k1["mp_desc"][s]
    # the octave gate at the clamped levels: the winner at the predicted level, perfect descriptors one above and two below it
    for s in S_GATES:
        L = L2[s]
        g = dict(q=float(q2[s]), level=L, winner=add(c2[s] + (1.5, -1.0), L, _flip(rng, d(s), 12)), above=None, below=None)
        if L + 1 < n_levels:
            g["above"] = add(c2[s] + (-1.0, 1.2), L + 1, d(s).copy())
        if L - 2 >= 0:
            g["below"] = add(c2[s] + (0.8, 1.4), L - 2, d(s).copy())
        named["gates"][s] = g
    # th: a key point inside the box at this candidate's th and outside it at the next smaller th; a perfect one outside the box
    # at this th and inside it at the next larger.  Sources: the first special slots whose surroundings are filed.
    free = [s for s in S_SPECIAL if filed(c2[s] - 13.0 * float(sf[L2[s]])) and filed(c2[s] + 13.0 * float(sf[L2[s]]))]
    smaller, larger = [t for t in THS if t < th], [t for t in THS if t > th]
    if smaller:
        s = free.pop(0)
        named["th_in"] = (s, add(c2[s] + (0.5 * (smaller[-1] + th) * float(sf[L2[s]]), 0.3), L2[s], _flip(rng, d(s), 6)))
    if larger:
        s = free.pop(0)
        add(c2[s] + (0.5 * (larger[0] + th) * float(sf[L2[s]]), -0.4), L2[s], d(s).copy())
        named["th_out"] = (s, add(c2[s] + (1.0, 1.0), L2[s], _flip(rng, d(s), 9)))
    if (cols, rows) == (1, 1):
        # a tie of two key points 12 pixels apart in x: in this grid both lie in cell (0, 0) and the lower index is first; in a
        # 64 x 48 grid over the same image the one with the smaller x is
        s = free.pop(0)
        a = add(c2[s] + (6.0, -1.0), L2[s], _flip(rng, d(s), 7))
        named["tie"] = (s, a, add(c2[s] + (-6.0, 1.0), L2[s], _flip(rng, d(s), 7)))
    while len(rows_) < N2_MIXED:
        uv = rng.uniform((min_x + 1, min_y + 1), (max_x - 1, max_y - 1))
        lvl = int(rng.integers(1, N_LEVELS - 1))
        pt = None if len(rows_) % 3 == 0 else dict(Z=_unpix(uv + rng.normal(size=2) * 3, rng.uniform(3.0, 8.0)), q=lvl - 0.5, wide=False, d1=None,
                                                   desc=rng.integers(0, 256, 32).astype(np.uint8))
        add(uv, int(rng.integers(0, n_levels)), rng.integers(0, 256, 32).astype(np.uint8), pt)
    n2 = len(rows_)
    fr = dict(bounds=spec["bounds"], grid=grid, log_scale=log_scale, scale_factors=sf, Rcw=R2.astype(f32), tcw=t2.astype(f32), **_mp_fields(n2))
    kp, octave, desc = np.zeros((n2, 2), f32), np.zeros(n2, np.int32), np.zeros((n2, 32), np.uint8)
    for j, (uv, o, de, pt) in enumerate(rows_):
        kp[j], octave[j], desc[j] = uv, o, de
        if pt is None:
            fr["has_point"][j] = 0
            continue
        _set_point(fr, j, pt["Z"], 0, pt["desc"], R2, t2)
        d1 = pt["d1"] or float(np.linalg.norm(s12 * (R12 @ pt["Z"]) + t12))     # the distance seen from key frame 1
        fr["dist_max"][j] = f32(d1 * float(SCALE) ** pt["q"])
        fr["dist_max_inv"][j], fr["dist_min_inv"][j] = f32(1.2) * fr["dist_max"][j], f32(0.8) * f32(fr["dist_max"][j] / SF[-1])
        if pt["wide"]:
            fr["dist_min_inv"][j], fr["dist_max_inv"][j] = f32(0.01), f32(1000.0)
    fr.update(kp=kp, octave=octave, desc=desc)
    pre1, pre2 = np.zeros(N1, np.uint8), np.zeros(n2, np.uint8)
    pre1[5], pre2[3], pre1[9] = 1, 1, 1
    return dict(kf2=fr, K=K.astype(f32), s12=f32(s12), R12=R12.astype(f32), t12=t12.astype(f32), th=f32(th), pre1=pre1, pre2=pre2,
                kind="mixed", small=False, named=named, name=spec["name"])


@functools.lru_cache(maxsize=None)
def pool_mixed():
    """the mixed candidates (inputs only; treat as read-only); all share key_frame_1()"""
    return [make_mixed(i) for i in range(len(POOL_MIXED))]


@functools.lru_cache(maxsize=None)
def pool_mixed_results(flavour, traversal="grid", mutant=None):
    return [search(key_frame_1(), c, flavour, traversal, tgt1=target_1(), mutant=mutant, first=pool_mixed()[0]) for c in pool_mixed()]


@functools.lru_cache(maxsize=None)
def pool_mutant_results(mutant):
    """POOL under a mutant: the brute traversal, float64"""
    return [search(key_frame_1(), c, "f64", "brute", tgt1=target_1(), mutant=mutant, first=pool()[0]) for c in pool()]


@functools.lru_cache(maxsize=None)
def measured_mixed():
    """CPU: as measured(), over the mixed pool"""
    worst = 0.0
    for a, b in zip(pool_mixed_results("f32"), pool_mixed_results("f64")):
        for d, diff in zip((1, 2), disagreements(a, b)):
            if diff.any():
                worst = max(worst, float(b["knife%d" % d][diff].max()))
    return worst


def band_mixed():
    """what tests/test_gpu_search_sim3.py leaves undecided on the mixed pool: 4 x its measured band"""
    return 4 * measured_mixed()
