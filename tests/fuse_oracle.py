"""A numpy restatement of the MATCH PHASE of both ORBmatcher::Fuse overloads (reference src/ORBmatcher.cc:825-975 and :977-1100 with
KeyFrame::GetFeaturesInArea / IsInImage, MapPoint::PredictScale and Frame::PosInGrid), the yardstick of qsp_fuse_batch, the
fixtures its tests share, and a small model of the ACTION phase for the shim test.  Written here from the formulas.

The arithmetic is the reference's float32 ("f32" in tests/search_sim3_oracle.py, whose helpers are used): cv::Mat products are row
sums in double rounded to float32 once with t added in float32, 1 / z is rounded to float32 once, u = fx * x + cx is a float32
multiply and a float32 add, ur = u - bf * invz, cv::norm(PO) and PO.dot(Pn) are summed in double, the chi-square product is float32
and compared in double.  Two traversals: "grid" walks a real mGrid as GetFeaturesInArea does (`dist < bestDist`), "brute" keeps the
minimum of the key dist << 40 | cell x << 33 | cell y << 26 | index -- the form of csrc/fuse.hpp.

Per pair the restatement also returns the KNIFE-EDGE DISTANCE, the smallest relative distance of any decision to its threshold:
|z| / |p| against 0; u, v against the four bounds (relative to the extent); dist3D against both limits; |PO.Pn - 0.5 dist3D| /
dist3D; log(ratio) / log_scale against the integers at which the clamped level changes; for every filed key point ||dx| - r| / r,
||dy| - r| / r and the ends of the visited cell range; for every key point that reaches the reprojection test |e2 * invSigma2 -
7.8 (5.99)| / 7.8 (5.99); |bestDist - 50.5| / 50.5.  A fixture names its deliberately exact pairs; every other pair must stay
above the threshold tests/test_gpu_search_sim3.py uses (so.band(), so.band_mixed())."""
import functools
import os

import numpy as np

from tests import search_sim3_oracle as so
from tests.search_sim3_oracle import _flip, _rot, _rowdot, f32, f64

TH_LOW = 50
MATCHED, Z_NEG, OUTSIDE, DISTANCE, ANGLE, EMPTY, NONE_ELIGIBLE, ABOVE_TH = range(8)
REASONS = ("matched", "z_neg", "outside", "distance", "angle", "empty", "none_eligible", "above_th")
MUTANTS = ("pose0", "K0", "no_bf", "stereo_always", "zero_mono", "chi_ge", "th_lt", "gate_unclamped", "tie_lowest", "list_as_pool")
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fuse_margins.json")


def threshold():
    """the knife-edge distance below which the Sim3 tests leave a slot undecided; here no pair may be that close"""
    return max(so.band(), so.band_mixed())


def match(T, pool, traversal="grid", mutant=None, first=None):
    """The match phase of Fuse(T, points of pool listed in T["list"]).  Returns dict(best_idx, best_dist, reason, level (one per
    listed pair), knife, info).  `mutant` (brute traversal only) makes ONE mistake a kernel or a staging loop could make: the pose
    (Rcw, tcw, Ow) or K of `first`, the batch's target 0; mbf dropped; the stereo test applied when u_right < 0; u_right == 0 taken
    as monocular; >= for > at the chi-square test; < for <= at 50; the octave window on the unclamped level; a tie to the lowest
    index; the list position used as the pool index.  The knife-edge distances are the true ones."""
    assert mutant is None or (mutant in MUTANTS and traversal == "brute")
    tgt = so._target(T)
    lst = np.asarray(T["list"], np.int64).reshape(-1)
    n_pair = len(lst)
    P = first if mutant == "pose0" else T
    R, t, Ow = np.asarray(P["Rcw"], f32).reshape(3, 3), np.asarray(P["tcw"], f32).reshape(3), np.asarray(P["Ow"], f32).reshape(3)
    K = np.asarray((first if mutant == "K0" else T)["K"], f32).reshape(5)
    bf = f32(0) if mutant == "no_bf" else K[4]
    th = f32(T["th"])
    min_x, max_x, min_y, max_y = [f32(b) for b in T["bounds"]]
    cols, rows, w_inv, h_inv = int(T["grid"][0]), int(T["grid"][1]), f32(T["grid"][2]), f32(T["grid"][3])
    sf, n_levels, log_scale = np.asarray(T["scale_factors"], f32), int(np.size(T["scale_factors"])), f32(T["log_scale"])
    inv_s2 = np.asarray(T["inv_level_sigma2"], f32).reshape(-1)
    kx, ky, kr = tgt["kp"][:, 0], tgt["kp"][:, 1], np.asarray(T["u_right"], f32).reshape(-1)
    octave, filed = tgt["octave"], tgt["ok"]
    Xw_all, Pn_all = np.asarray(pool["Xw"], f32).reshape(-1, 3), np.asarray(pool["normal"], f32).reshape(-1, 3)
    mp_desc = np.asarray(pool["desc"], np.uint8).reshape(-1, 32)
    best, dist = np.full(n_pair, -1, np.int64), np.full(n_pair, -1, np.int64)
    reason, level_out, knife, info = np.zeros(n_pair, np.int64), np.full(n_pair, -1, np.int64), np.full(n_pair, np.inf), {}
    for a in range(n_pair):
        i = int(lst[a])
        if mutant == "list_as_pool":
            i = a % len(Xw_all)
        X, Pn = Xw_all[i], Pn_all[i]
        with np.errstate(all="ignore"):
            p = _rowdot(R, X, f32) + t
            invz = f32(1.0 / f64(p[2]))
            x, y = p[0] * invz, p[1] * invz
            u, v = K[0] * x + K[2], K[1] * y + K[3]
            ur = u - bf * invz
            PO = X - Ow
            d3 = f32(np.sqrt((f64(PO[0]) * f64(PO[0]) + f64(PO[1]) * f64(PO[1])) + f64(PO[2]) * f64(PO[2])))
            dot = (f64(PO[0]) * f64(Pn[0]) + f64(PO[1]) * f64(Pn[1])) + f64(PO[2]) * f64(Pn[2])
            k = [abs(float(p[2])) / max(float(np.linalg.norm(p.astype(f64))), 1e-30)]
            if p[2] < 0:
                reason[a], knife[a] = Z_NEG, k[0]
                continue
            k += [abs(float(u) - float(b)) / float(max_x - min_x) for b in (min_x, max_x)]
            k += [abs(float(v) - float(b)) / float(max_y - min_y) for b in (min_y, max_y)]
            if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
                reason[a], knife[a] = OUTSIDE, np.nanmin(k)
                continue
            dmin, dmaxi = f32(pool["dist_min_inv"][i]), f32(pool["dist_max_inv"][i])
            k += [abs(float(d3) - float(dmin)) / float(dmin), abs(float(d3) - float(dmaxi)) / float(dmaxi)]
            if d3 < dmin or d3 > dmaxi:
                reason[a], knife[a] = DISTANCE, min(k)
                continue
            k.append(abs(float(dot) - 0.5 * float(d3)) / float(d3))
            if dot < 0.5 * f64(d3):
                reason[a], knife[a] = ANGLE, min(k)
                continue
            ratio = f32(pool["dist_max"][i]) / d3
            q = np.log(ratio) / log_scale                         # (numpy's float32 log stands in for logf)
            k += [abs(float(q) - e) for e in range(n_levels - 1)]
            fl = np.ceil(q)
            level = gate = 0 if fl < 0 else (n_levels - 1 if fl >= n_levels else int(fl))
            if mutant == "gate_unclamped":
                gate = int(fl)
            level_out[a] = level
            r = th * sf[level]
            a_x, b_x, a_y, b_y = ((u - min_x) - r) * w_inv, ((u - min_x) + r) * w_inv, ((v - min_y) - r) * h_inv, ((v - min_y) + r) * h_inv
            lo_x, hi_x, lo_y, hi_y = int(np.floor(a_x)), int(np.ceil(b_x)), int(np.floor(a_y)), int(np.ceil(b_y))
            min_cx, max_cx, min_cy, max_cy = max(0, lo_x), min(cols - 1, hi_x), max(0, lo_y), min(rows - 1, hi_y)
            dx, dy = np.abs(kx - u), np.abs(ky - v)
            if filed.any():
                cx, cy = tgt["cx"][filed].astype(f64), tgt["cy"][filed].astype(f64)
                k += [float(np.min(np.abs(dx[filed] - r) / r)), float(np.min(np.abs(dy[filed] - r) / r)),
                      float(np.min(np.abs(f64(a_x) - (cx + 1)))), float(np.min(np.abs(f64(b_x) - (cx - 1)))),
                      float(np.min(np.abs(f64(a_y) - (cy + 1)))), float(np.min(np.abs(f64(b_y) - (cy - 1))))]
            in_box = (dx < r) & (dy < r)
            no_range = min_cx >= cols or max_cx < 0 or min_cy >= rows or max_cy < 0
            if traversal == "grid":
                found = []
                if not no_range:
                    for ix in range(min_cx, max_cx + 1):
                        for iy in range(min_cy, max_cy + 1):
                            found += [j for j in tgt["grid"][ix][iy] if in_box[j]]
                found = np.array(found, np.int64)
            else:
                elig = filed & (tgt["cx"] >= min_cx) & (tgt["cx"] <= max_cx) & (tgt["cy"] >= min_cy) & (tgt["cy"] <= max_cy) & in_box
                found = np.nonzero(elig)[0] if not no_range else np.zeros(0, np.int64)
            inf = dict(q=float(q), level=level, u=float(u), v=float(v), ur=float(ur), r=float(r), d3=float(d3), n_found=len(found), tie=False,
                       tie_same_cell=False, chi={}, stereo_kept=0, mono_kept=0)
            info[a] = inf
            if len(found) == 0:
                reason[a], knife[a] = EMPTY, min(k)
                continue
            octs = octave[found]
            keep = found[(octs >= gate - 1) & (octs <= gate)]
            if T["check"] and len(keep):                            # :914-938
                ex, ey = u - kx[keep], v - ky[keep]
                e2 = ex * ex + ey * ey
                stereo = kr[keep] > 0 if mutant == "zero_mono" else kr[keep] >= 0
                if mutant == "stereo_always":
                    stereo = np.ones(len(keep), bool)
                er = ur - kr[keep]
                e2 = np.where(stereo, e2 + er * er, e2).astype(f32)
                val = (e2 * inv_s2[np.clip(octave[keep], 0, len(inv_s2) - 1)]).astype(f64)
                thr = np.where(stereo, 7.8, 5.99)
                k.append(float(np.min(np.abs(val - thr) / thr)))
                inf["chi"] = {int(j): (float(w), float(h)) for j, w, h in zip(keep, val, thr)}
                ok = ~(val >= thr) if mutant == "chi_ge" else ~(val > thr)
                inf["stereo_kept"], inf["mono_kept"] = int((ok & stereo).sum()), int((ok & ~stereo).sum())
                keep = keep[ok]
            if len(keep) == 0:
                reason[a], knife[a] = NONE_ELIGIBLE, min(k)
                continue
            hd = so.popcount_rows(tgt["desc"][keep], mp_desc[i])
            if traversal == "grid":
                b, bd = -1, 256
                for j, d in zip(keep, hd):                          # `dist < bestDist`: the first of the traversal stays
                    if d < bd:
                        b, bd = int(j), int(d)
            else:
                key = (hd << 40) | (tgt["cx"][keep] << 33) | (tgt["cy"][keep] << 26) | keep
                if mutant == "tie_lowest":
                    key = (hd << 40) | keep
                kmin = int(key.min())
                b, bd = kmin & ((1 << 26) - 1), kmin >> 40
            k.append(abs(bd - 50.5) / 50.5)
            knife[a] = min(k)
            dist[a] = bd
            if (bd < TH_LOW) if mutant == "th_lt" else (bd <= TH_LOW):
                best[a] = b
            else:
                reason[a] = ABOVE_TH
            ties = keep[hd == bd]
            if len(ties) > 1:
                inf["tie"] = int(ties.min()) != b                  # the lowest index is not the traversal's first
                inf["tie_same_cell"] = len({(int(tgt["cx"][j]), int(tgt["cy"][j])) for j in ties}) < len(ties)
    return dict(best_idx=best, best_dist=dist, reason=reason, level=level_out, knife=knife, info=info)


def match_all(targets, pool, traversal="grid", mutant=None):
    return [match(T, pool, traversal, mutant, first=targets[0]) for T in targets]


def differs(a, b):
    return (a["best_idx"] != b["best_idx"]) | (a["best_dist"] != b["best_dist"]) | (a["reason"] != b["reason"]) | (a["level"] != b["level"])


# ---- the main scene: targets that differ from each other around one shared pool -------------------------------------------------
N_COMMON = 96
SPEC = [   # n: key points
    dict(name="8 levels at 1.2, VGA 64 x 48", n=300, levels=8, scale=1.2, th=3.0, bounds=(0.0, 640.0, 0.0, 480.0), grid=(64, 48),
         K=(517.3, 516.5, 318.6, 255.3, 40.0), seed=1),
    dict(name="5 levels at 1.5, 5 x 7 grid", n=129, levels=5, scale=1.5, th=4.0, bounds=(0.0, 640.0, 0.0, 480.0), grid=(5, 7),
         K=(480.0, 485.0, 300.5, 230.25, 35.5), seed=2),
    dict(name="16 levels at 1.1, bounds off 0, 64 x 64", n=200, levels=16, scale=1.1, th=5.0, bounds=(-12.5, 651.25, -8.25, 487.5), grid=(64, 64),
         K=(545.0, 540.0, 335.0, 244.0, 44.25), seed=3),
]
BASE_SCALE, BASE_LEVELS = 1.2, 8
# reserved image zones of every target of the scene: no random key point falls in x < ZONE_X
ZONE_X = 120.0
# pool slots beyond the common points (all placed in the base camera, which every target's pose is close to)
P_BEHIND, P_OUT_U, P_OUT_V, P_NEAR, P_FAR, P_AWAY, P_SIDE, P_EMPTY, P_WRONG_OCT, P_ABOVE, P_CHI, P_ZERO_UR = range(N_COMMON, N_COMMON + 12)
N_POOL = N_COMMON + 12
ZONE_UV = {P_EMPTY: (40.0, 60.0), P_WRONG_OCT: (40.0, 140.0), P_ABOVE: (40.0, 220.0), P_CHI: (40.0, 300.0), P_ZERO_UR: (40.0, 380.0)}
ZONE_LEVEL = 2
BASE_K = np.array([517.3, 516.5, 318.6, 255.3], f64)


def _unpix(K, uv, z):
    return np.array([(uv[0] - K[2]) / K[0] * z, (uv[1] - K[3]) / K[1] * z, z])


def _pixk(K, Y):
    return np.array([K[0] * Y[0] / Y[2] + K[2], K[1] * Y[1] / Y[2] + K[3]])


@functools.lru_cache(maxsize=None)
def main_pool():
    """the shared pool (treat as read-only): points in front of a base camera at the origin"""
    rng = np.random.default_rng(7711)
    uv = np.stack([rng.uniform(170, 590, N_POOL), rng.uniform(50, 430, N_POOL)], -1)
    for p, c in ZONE_UV.items():
        uv[p] = c
    z = rng.uniform(4.0, 8.0, N_POOL)
    Y = np.stack([_unpix(BASE_K, uv[i], z[i]) for i in range(N_POOL)])
    Y[P_BEHIND] = (0.3, 0.2, -3.0)
    Y[P_OUT_U], Y[P_OUT_V] = _unpix(BASE_K, (-400.0, 200.0), 5.0), _unpix(BASE_K, (300.0, 1100.0), 5.0)
    level = rng.integers(1, 6, N_POOL)
    level[list(ZONE_UV)] = ZONE_LEVEL
    d = np.linalg.norm(Y, axis=1)
    normal = Y / d[:, None]                                        # seen from the origin: PO.Pn is about dist3D
    normal[P_AWAY] = -normal[P_AWAY]                               # faces away
    side = np.cross(Y[P_SIDE], (0.0, 1.0, 0.0))
    normal[P_SIDE] = side / np.linalg.norm(side)                   # seen edge-on: PO.Pn is about 0
    dist_max = (d * BASE_SCALE ** (level + 0.5)).astype(f32)
    pool = dict(Xw=Y.astype(f32), normal=normal.astype(f32), dist_max=dist_max, dist_max_inv=f32(1.2) * dist_max,
                dist_min_inv=f32(0.8) * (dist_max / f32(BASE_SCALE ** (BASE_LEVELS - 1))).astype(f32),
                desc=rng.integers(0, 256, (N_POOL, 32)).astype(np.uint8), level=level)
    pool["dist_min_inv"][P_NEAR] = f32(50.0)
    pool["dist_max_inv"][P_FAR] = f32(0.5)
    return pool


def make_target(spec, n=None, check=True, lst=None):
    """A target of the main scene: its own pose near the base camera, camera, pyramid, grid and th.  A key point sits about half a
    pixel from the projection of every common point it sees (octave: the level predicted with THIS pyramid or one below; every
    second one stereo with u_right next to the point's own), then the hand-made ones of the reserved zones, then unrelated key
    points up to n.  With n below that, the first n are kept."""
    pool = main_pool()
    n = spec["n"] if n is None else n
    rng = np.random.default_rng(88000 + spec["seed"])
    R = _rot(rng, 0.03).astype(f32)
    t = (rng.normal(size=3) * 0.12).astype(f32)
    R64, t64 = R.astype(f64), t.astype(f64)
    Ow = (-(R64.T @ t64)).astype(f32)
    K = np.array(spec["K"], f32)
    K64 = K.astype(f64)
    levels, scale = spec["levels"], f32(spec["scale"])
    sf, log_scale = np.array([scale ** i for i in range(levels)], f32), f32(np.log(scale))
    min_x, max_x, min_y, max_y = spec["bounds"]
    cols, rows = spec["grid"]
    grid = (cols, rows, f32(cols) / f32(max_x - min_x), f32(rows) / f32(max_y - min_y))
    rows_ = []                                                     # (uv, octave, desc, u_right)

    def see(i):
        Y = R64 @ pool["Xw"][i].astype(f64) + t64
        uv = _pixk(K64, Y)
        d3 = np.linalg.norm(pool["Xw"][i].astype(f64) - Ow.astype(f64))
        q = np.log(float(pool["dist_max"][i]) / d3) / float(log_scale)
        L = int(min(max(np.ceil(q), 0), levels - 1))
        return uv, float(uv[0] - float(K64[4]) / Y[2]), L

    def add(uv, octave, desc, u_right):
        rows_.append((np.asarray(uv, f64), int(octave), desc, float(u_right)))
        return len(rows_) - 1

    named = {}
    for i in rng.permutation(N_COMMON):
        uv, ur, L = see(int(i))
        if not (ZONE_X + 30 < uv[0] < max_x - 20 and min_y + 20 < uv[1] < max_y - 20):
            continue
        stereo = len(rows_) % 2 == 0
        add(uv + rng.normal(size=2) * 0.4, max(L - int(rng.integers(0, 2)), 0), _flip(rng, pool["desc"][i], int(rng.integers(0, 12))),
            ur + rng.normal() * 0.3 if stereo else -1.0)
    # the reserved zones: each hand-made case alone in its box
    d = lambda p: pool["desc"][p]
    uv, ur, L = see(P_WRONG_OCT)                                  # perfect descriptors two levels below and one above: none eligible
    if L - 2 >= 0:
        add(uv + (0.5, 0.3), L - 2, d(P_WRONG_OCT).copy(), -1.0)
    named["wrong_oct"] = add(uv + (-0.4, 0.2), min(L + 1, levels - 1) if L + 1 < levels else 0, d(P_WRONG_OCT).copy(), -1.0)
    uv, ur, L = see(P_ABOVE)                                      # a lone key point at Hamming distance 80
    named["above"] = add(uv + (0.3, -0.3), L, _flip(rng, d(P_ABOVE), 80), -1.0)
    uv, ur, L = see(P_CHI)                                        # inside the box, outside both chi-square limits: 0.95 r away at its level
    named["chi"] = add(uv + (0.95 * spec["th"] * float(sf[L]), 0.0), L, d(P_CHI).copy(), -1.0)
    uv, ur, L = see(P_ZERO_UR)                                    # u_right == 0.0 is stereo: er = ur is tens of pixels
    named["zero_ur"] = add(uv + (0.2, 0.2), L, d(P_ZERO_UR).copy(), 0.0)
    while len(rows_) < n:
        uv = rng.uniform((ZONE_X + 20, min_y + 1), (max_x - 1, max_y - 1))
        add(uv, int(rng.integers(0, levels)), rng.integers(0, 256, 32).astype(np.uint8), uv[0] - rng.uniform(2, 30) if len(rows_) % 3 == 0 else -1.0)
    rows_ = rows_[:n]
    kp = np.array([r[0] for r in rows_], f32).reshape(-1, 2)
    T = dict(name=spec["name"], bounds=spec["bounds"], grid=grid, log_scale=log_scale, scale_factors=sf, Rcw=R, tcw=t, Ow=Ow, K=K, th=f32(spec["th"]),
             kp=kp, octave=np.array([r[1] for r in rows_], np.int32), desc=np.array([r[2] for r in rows_], np.uint8).reshape(-1, 32),
             u_right=np.array([r[3] for r in rows_], f32), inv_level_sigma2=(f32(1) / (sf * sf)).astype(f32), check=bool(check),
             list=np.arange(N_POOL, dtype=np.int32) if lst is None else np.asarray(lst, np.int32), named=named)
    return T


@functools.lru_cache(maxsize=None)
def main_targets():
    """three targets with different n, n_levels, grids, K, th and pose; the pose overload (mono and stereo key points mixed), the
    second one listing the pool in a permuted order and the third only every second point"""
    rng = np.random.default_rng(515)
    return [make_target(SPEC[0]), make_target(SPEC[1], lst=rng.permutation(N_POOL)), make_target(SPEC[2], lst=np.arange(0, N_POOL, 2)[::-1])]


@functools.lru_cache(maxsize=None)
def sim3_targets():
    """the same frames under the Sim3 overload: no reprojection test"""
    return [dict(T, check=False) for T in main_targets()]


STRIDE_N = (0, 1, 63, 64, 65, 4097)


@functools.lru_cache(maxsize=None)
def stride_targets():
    """the lane-stride and reduction edges: targets of 0, 1, 63, 64, 65 and 4097 key points"""
    return [make_target(dict(SPEC[0], seed=10 + k), n=n) for k, n in enumerate(STRIDE_N)]


# ---- the exact scene: every value chosen so that float32 arithmetic lands ON the threshold --------------------------------------
# R is the identity with -0.0 in the third row's zeros and tcw = (0, 0, -0.0): z is exactly the point's third coordinate, sign of
# zero included.  fx = fy = 512, z = 4: u = 128 * X + 320 exactly.  5 levels at 1.5 (scale factors exact in float32), th = 4:
# radius 4, 6, 9, 13.5, 20.25.  Each case sits alone in a box; boxes are 50 pixels apart.
E_K = (512.0, 512.0, 320.0, 240.0, 64.0)
E_LEVELS, E_SCALE, E_TH, E_Z = 5, 1.5, 4.0, 4.0


def _next(x, up=True):
    return np.nextafter(f32(x), f32(np.inf if up else -np.inf))


@functools.lru_cache(maxsize=None)
def exact_scene():
    """Returns (targets, pool, cases): targets[0] the pose overload, targets[1] the same frame under the Sim3 overload; cases maps
    a name to (target, list position, what must come out) with `exact`: the pairs that sit ON a threshold."""
    rng = np.random.default_rng(9191)
    sf = np.array([f32(E_SCALE) ** i for i in range(E_LEVELS)], f32)
    log_scale = f32(np.log(f32(E_SCALE)))
    inv_s2 = (f32(1) / (sf * sf)).astype(f32)
    R = np.array([[1, 0, 0], [0, 1, 0], [-0.0, -0.0, 1]], f32)
    t = np.array([0, 0, -0.0], f32)
    pts, kps = [], []                                              # pool rows, key-point rows
    cases = {}
    boxes = iter([(60.0 + 50.0 * (k % 11), 40.0 + 50.0 * (k // 11)) for k in range(88)])

    def point(uv, level=1, q_off=-0.5, z=E_Z, desc=None):
        """a pool point projecting exactly to uv (multiples of 1/64) whose predicted level is `level`"""
        X = np.array([(uv[0] - 320.0) / 128.0 * (z / E_Z), (uv[1] - 240.0) / 128.0 * (z / E_Z), z], f32)
        d3 = f32(np.sqrt((f64(X[0]) * f64(X[0]) + f64(X[1]) * f64(X[1])) + f64(X[2]) * f64(X[2])))
        dmax = f32(float(d3) * E_SCALE ** (level + q_off))
        nrm = (X.astype(f64) / float(d3)).astype(f32)
        pts.append(dict(Xw=X, normal=nrm, dist_max=dmax, dist_max_inv=f32(1.2) * dmax, dist_min_inv=f32(0.8) * f32(dmax / sf[-1]),
                        desc=rng.integers(0, 256, 32).astype(np.uint8) if desc is None else desc, d3=d3))
        return len(pts) - 1

    def kpt(uv, octave, desc, u_right=-1.0):
        kps.append((np.array(uv, f32), int(octave), desc, f32(u_right)))
        return len(kps) - 1

    def case(name, p, **want):
        cases[name] = dict(point=p, **want)

    # TH_LOW: a lone key point at distance exactly 50, and one at exactly 51
    for name, nb, hit in (("th_50", 50, True), ("th_51", 51, False)):
        c = next(boxes)
        p = point(c)
        j = kpt((c[0] + 0.5, c[1] - 0.25), 1, _flip(rng, pts[p]["desc"], nb))
        case(name, p, best=j if hit else -1, dist=nb, reason=MATCHED if hit else ABOVE_TH, exact=True)
    # |dx| == radius exactly (level 1: radius 6): outside the strict box; one float32 step nearer: inside
    for name, hit in (("dx_eq_r", False), ("dx_below_r", True)):
        c = next(boxes)
        p = point(c)
        kx = f32(c[0] + 6.0) if not hit else _next(c[0] + 6.0, False)
        assert (abs(kx - f32(c[0])) == f32(6.0)) != hit
        j = kpt((kx, c[1]), 1, pts[p]["desc"].copy())
        case(name, p, best=j if hit else -1, dist=0 if hit else -1, reason=MATCHED if hit else EMPTY, exact=True, sim3_only=True)
    # u == max_x exactly: outside (half open); one step below: inside; u == min_x: inside
    for name, uv, inside in (("u_eq_max", (640.0, 240.0), False), ("u_below_max", (float(_next(640.0, False)), 240.0), True), ("u_eq_min", (0.0, 300.0), True)):
        p = point(uv)
        if name == "u_below_max":
            pts[p]["Xw"][0] = f32(2.5 - 2.0 ** -21)                # 128 * (2.5 - 2^-21) + 320 is the float32 below 640
        case(name, p, reason=EMPTY if inside else OUTSIDE, exact=True)
    # z == +0.0 and z == -0.0: 1 / z is +inf / -inf, u is not finite: outside the image, never `z < 0`
    for name, z in (("z_plus_0", 0.0), ("z_minus_0", -0.0)):
        p = point((400.0, 300.0))
        pts[p]["Xw"][2] = f32(z)
        case(name, p, reason=OUTSIDE, exact=True)
    p = point((400.0, 300.0))
    pts[p]["Xw"][2] = -np.finfo(f32).tiny                          # the smallest normal negative float32: z < 0
    case("z_tiny_neg", p, reason=Z_NEG, exact=True)
    # dist3D equal to a limit passes (strict compares); one step inside the limit refuses
    for name, which, step, ok in (("d_eq_min", "dist_min_inv", 0, True), ("d_eq_max", "dist_max_inv", 0, True),
                                  ("d_below_min", "dist_min_inv", 1, False), ("d_above_max", "dist_max_inv", -1, False)):
        c = next(boxes)
        p = point(c)
        d3 = pts[p]["d3"]
        pts[p][which] = d3 if step == 0 else _next(d3, step > 0)
        j = kpt((c[0] + 0.5, c[1] + 0.5), 1, _flip(rng, pts[p]["desc"], 3))
        case(name, p, best=j if ok else -1, dist=3 if ok else -1, reason=MATCHED if ok else DISTANCE, exact=True)
    # the level clamped at 0 (log(ratio) / log_scale = -2.6: the window's lower edge is -1) and at n_levels - 1 (7.3): the octave
    # window is the CLAMPED level's; perfect descriptors wait one level outside it
    for name, q, L in (("clamp_0", -2.6, 0), ("clamp_top", 7.3, E_LEVELS - 1)):
        c = next(boxes)
        p = point(c, level=0, q_off=q)
        pts[p]["dist_min_inv"], pts[p]["dist_max_inv"] = f32(0.01), f32(1000.0)
        j = kpt((c[0] + 0.5, c[1] - 0.5), L, _flip(rng, pts[p]["desc"], 9))
        kpt((c[0] - 0.5, c[1] + 0.5), 1 if L == 0 else L - 2, pts[p]["desc"].copy())
        case(name, p, best=j, dist=9, reason=MATCHED, level=L, exact=False)
    # the chi-square limits: a lone key point whose e2 * invSigma2 is the float32 value just below / just above 5.99 (mono, ey = 0)
    # and 7.8 (stereo with u_right == ur exactly: er = 0).  Found by stepping kx one float32 at a time.
    for name, thr, stereo in (("chi_mono", 5.99, False), ("chi_stereo", 7.8, True)):
        for side in ("in", "out"):
            c = next(boxes)
            p = point(c)
            u, inv = f32(c[0]), inv_s2[1]
            kx = f32(c[0] - np.sqrt(thr / float(inv)) + 0.01)
            val = lambda x: float(f32((u - x) * (u - x)) * inv)
            while val(kx) <= thr:
                kx = _next(kx, False)
            if side == "in":
                kx = _next(kx)
                assert val(kx) <= thr < val(_next(kx, False))
            ur = f32(u - f32(E_K[4]) * f32(1.0 / E_Z))
            j = kpt((kx, c[1]), 1, _flip(rng, pts[p]["desc"], 5), ur if stereo else -1.0)
            hit = side == "in"
            case("%s_%s" % (name, side), p, best=j if hit else -1, dist=5 if hit else -1, reason=MATCHED if hit else NONE_ELIGIBLE, exact=True,
                 pose_only=True, chi=(j, thr))
    # ties.  two cells: x = 10 * cell - 5 .. 10 * cell + 5; the LOWER index lies in the larger cell x, the walk's first is the higher
    c = (205.0, 390.0)
    p = point(c)
    a = kpt((c[0] + 1.0, c[1] + 0.5), 1, _flip(rng, pts[p]["desc"], 7))
    b = kpt((c[0] - 1.0, c[1] - 0.5), 1, _flip(rng, pts[p]["desc"], 7))
    case("tie_cx", p, best=b, dist=7, reason=MATCHED, lowest=a, exact=False)
    c = (262.0, 335.0)                                             # same cell x, the lower index in the larger cell y
    p = point(c)
    a = kpt((c[0] + 0.5, c[1] + 1.0), 1, _flip(rng, pts[p]["desc"], 6))
    b = kpt((c[0] - 0.5, c[1] - 1.0), 0, _flip(rng, pts[p]["desc"], 6))
    case("tie_cy", p, best=b, dist=6, reason=MATCHED, lowest=a, exact=False)
    c = (321.0, 283.0)                                             # within one cell: the lower index is the first
    p = point(c)
    a = kpt((c[0] + 0.5, c[1] + 0.5), 1, _flip(rng, pts[p]["desc"], 4))
    b = kpt((c[0] - 0.5, c[1] - 0.5), 1, _flip(rng, pts[p]["desc"], 4))
    case("tie_cell", p, best=a, dist=4, reason=MATCHED, lowest=a, exact=False)
    pool = {k: np.array([q[k] for q in pts]) for k in ("Xw", "normal", "dist_max", "dist_max_inv", "dist_min_inv", "desc")}
    T = dict(name="exact", bounds=(0.0, 640.0, 0.0, 480.0), grid=(64, 48, f32(64) / f32(640), f32(48) / f32(480)), log_scale=log_scale,
             scale_factors=sf, Rcw=R, tcw=t, Ow=np.zeros(3, f32), K=np.array(E_K, f32), th=f32(E_TH),
             kp=np.array([k[0] for k in kps], f32), octave=np.array([k[1] for k in kps], np.int32),
             desc=np.array([k[2] for k in kps], np.uint8), u_right=np.array([k[3] for k in kps], f32), inv_level_sigma2=inv_s2, check=True,
             list=np.arange(len(pts), dtype=np.int32), named={})
    return [T, dict(T, check=False)], pool, cases


@functools.lru_cache(maxsize=None)
def results(which, traversal="grid", mutant=None):
    targets, pool = scene(which)
    return match_all(targets, pool, traversal, mutant)


def scene(which):
    if which == "exact":
        return exact_scene()[:2]
    return dict(main=main_targets, sim3=sim3_targets, stride=stride_targets)[which](), main_pool()


SCENES = ("main", "sim3", "stride", "exact")


def exact_pairs(which):
    """(target, list position) of the pairs that sit ON a threshold by construction"""
    if which != "exact":
        return set()
    cases = exact_scene()[2]
    return {(k, c["point"]) for c in cases.values() if c["exact"] for k in (0, 1)}


# ---- the action phase: a model of the map for the shim test ----------------------------------------------------------------------
class MapModel:
    """Points with observation sets and bad flags, key frames with slots.  replace(dying, survivor): the survivor takes over every
    slot the dying point holds, unless it is observed in that key frame already (the slot is emptied then); the dying point is bad
    afterwards and observes nothing.  add(point, kf, idx): the point fills the empty slot and observes it."""

    def __init__(self, n_slots):
        self.slots = {kf: [None] * n for kf, n in n_slots.items()}
        self.obs, self.bad = {}, {}

    def point(self, p, bad=False):
        self.obs.setdefault(p, {})
        self.bad[p] = bad

    def add(self, p, kf, idx):
        self.slots[kf][idx] = p
        self.obs[p][kf] = idx

    def in_kf(self, p, kf):
        return kf in self.obs[p]

    def replace(self, dying, survivor):
        if dying == survivor:
            return
        for kf, idx in sorted(self.obs[dying].items()):
            if kf in self.obs[survivor]:
                self.slots[kf][idx] = None
            else:
                self.slots[kf][idx] = survivor
                self.obs[survivor][kf] = idx
        self.obs[dying] = {}
        self.bad[dying] = True

    def state(self):
        return dict(slots={k: list(v) for k, v in self.slots.items()}, bad=dict(self.bad), obs={p: dict(o) for p, o in self.obs.items()})


def fuse_pose_model(m, targets, points, answers):
    """FuseBatch, pose overload, on the model: answers[k][a] = (best_idx, best_dist) of target k's a-th LISTED point (listed from
    the state at entry).  Returns (n_fused per target, n_stale)."""
    lists = [[i for i, p in enumerate(points) if p is not None and not m.bad[p] and not m.in_kf(p, kf)] for kf in targets]
    survived, n_stale, fused = set(), 0, []
    for k, kf in enumerate(targets):
        n = 0
        for a, i in enumerate(lists[k]):
            p = points[i]
            if m.bad[p] or m.in_kf(p, kf):
                continue
            n_stale += p in survived
            best = answers[k][a][0]
            if best < 0:
                continue
            q = m.slots[kf][best]
            if q is not None:
                if not m.bad[q]:
                    if len(m.obs[q]) > len(m.obs[p]):
                        m.replace(p, q)
                        survived.add(q)
                    else:
                        m.replace(q, p)
                        survived.add(p)
            else:
                m.add(p, kf, best)
            n += 1
        fused.append(n)
    return fused, n_stale, lists


def fuse_sim3_model(m, targets, points, answers, apply_replacements=True):
    """FuseBatch, Sim3 overload: fills replace[k][i] and, between targets, applies the caller's block (the key frame's point is
    replaced BY the loop point) when apply_replacements.  Returns (n_fused, n_stale, lists, replace)."""
    lists = [[i for i, p in enumerate(points) if p is not None and not m.bad[p] and p not in set(m.slots[kf])] for kf in targets]
    survived, n_stale, fused, replace = set(), 0, [], []
    for k, kf in enumerate(targets):
        n, rep = 0, [None] * len(points)
        found = set(m.slots[kf])
        for a, i in enumerate(lists[k]):
            p = points[i]
            if m.bad[p] or p in found:
                continue
            n_stale += i in survived
            best = answers[k][a][0]
            if best < 0:
                continue
            q = m.slots[kf][best]
            if q is not None:
                if not m.bad[q]:
                    rep[i] = q
                    survived.add(i)
            else:
                m.add(p, kf, best)
            n += 1
        fused.append(n)
        replace.append(rep)
        if apply_replacements:
            for i, q in enumerate(rep):
                if q is not None:
                    m.replace(q, points[i])
    return fused, n_stale, lists, replace
