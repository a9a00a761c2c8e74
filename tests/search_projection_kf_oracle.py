"""A line-by-line SERIAL restatement in np.float32 of the two projection searches that fill one frame's slots from a list of map
points -- RELOC: ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
(reference src/ORBmatcher.cc:1472-1599) with Frame::GetFeaturesInArea; SIM3: SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const
vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, th) (:290-403) with KeyFrame::IsInImage and KeyFrame::GetFeaturesInArea --
with MapPoint::PredictScale and ComputeThreeMaxima: the yardstick of qsp_search_by_projection_kf, and the fixtures its tests share.
Written here from the formulas; the builder, the scenes and the helpers of tests/search_projection_oracle.py are used.

serial() walks the sources in order over a live slot table: a slot is skipped when it holds ANY point -- at entry
frame["slot_blocked"], afterwards every slot an earlier source was written to.  rounds() is a numpy version of the parallel iteration
of csrc/search_projection.hpp with every source blocking (claim[idx] = the smallest source that chose idx in the round before;
source i is blocked where claim[idx] < i) and returns its round count.

The arithmetic: cv::Mat products are row sums in double rounded to float32 once with t added in float32; RELOC (float)(1.0 / z) and u
= fx * xc * invzc + cx left to right; SIM3 1 / z in float32, x = X * invz, u = fx * x + cx; PO = P - Ow in float32, cv::norm(PO) and
PO.dot(Pn) summed in double; `PO.dot(Pn) < 0.5 * dist` compared in double; numpy's float32 log stands in for logf.

serial() counts every branch it takes (BRANCHES) and returns per source the KNIFE-EDGE DISTANCE, the smallest relative distance of
any float decision to its threshold: |z| / |p| (SIM3); u, v against the four bounds (relative to the extent); dist against both
limits; |dot - 0.5 dist| / dist (SIM3); log(ratio) / log_scale against the integers at which the clamped level changes (knife_q);
for the filed key points ||dx| - r| / r, ||dy| - r| / r and the ends of the cell range.  The only operation in which the device and
numpy may differ is logf (a few float32 ulp), so knife_q must keep THRESHOLD = 1e-4 levels from every integer, and no source other
than the deliberately exact ones may sit ON any threshold: its knife-edge distance stays above ON_THRESHOLD = 1e-6.

The taps: level, proj_x and proj_y are the predicted level and (u, v) of a source that passed every gate, else 0.

`mutant` makes ONE deliberate mistake (MUTANTS); tests/test_oracle_search_projection_kf.py shows that each changes an output."""
import collections
import functools
import os

import numpy as np

from tests import search_projection_oracle as po
from tests import search_sim3_oracle as so
from tests.search_projection_oracle import (ABOVE_TH, ANGLE, DISTANCE, EMPTY, HISTO_LENGTH, INVALID_SRC, MATCHED, NONE_ELIGIBLE, NONFINITE,
                                            ON_THRESHOLD, OUTSIDE, THRESHOLD, Z_NEG, _at, _next, _spread, rot_bin, three_maxima)
from tests.search_sim3_oracle import _rowdot, f32, f64

RELOC, SIM3 = 0, 1
MODES = (RELOC, SIM3)
MODE_NAME = {RELOC: "reloc", SIM3: "sim3"}
TH_LOW = 50
MUTANTS = ("reloc_z_neg", "image_half_open", "image_closed", "window_top_level", "window_top_plus1", "accept_lt", "accept_100", "right_test",
           "ratio_test", "non_blocking", "angle_le", "reloc_invz_order", "sim3_invz_order", "tie_cy_cx")
MUTANTS_OF = {RELOC: tuple(m for m in MUTANTS if m not in ("image_closed", "window_top_plus1", "angle_le", "sim3_invz_order")),
              SIM3: tuple(m for m in MUTANTS if m not in ("reloc_z_neg", "image_half_open", "window_top_level", "reloc_invz_order"))}
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "search_projection_kf_margins.json")
PER_SOURCE = ("choice", "dist", "reason", "level", "proj_x", "proj_y", "bin")
_COMMON = ("invalid", "outside", "nonfinite", "dist_near", "dist_far", "clamp_0", "clamp_top", "level_mid", "no_range", "area_empty",
           "blocked_initial", "blocked_by_source", "best_update", "no_update", "none_eligible", "above_th", "kept", "box_out", "unfiled")
BRANCHES = {RELOC: _COMMON + ("z_neg_searched", "level_out", "rot_neg", "bin_wrap", "bin_invalid", "nulled", "maxima", "ori_off"),
            SIM3: _COMMON + ("z_neg", "z_minus_0", "angle", "octave_skip")}


def decompose_scw(Scw):
    """:299-303 with cv::Mat on CV_32F: scw = (float)sqrt(row0 . row0) summed in double; the division by scw is a float32 product
    with (float)(1.0 / scw); Ow = -Rcw^T tcw with each row summed in double and rounded once"""
    S = np.asarray(Scw, f32)[:3, :4]
    scw = f32(np.sqrt((f64(S[0, 0]) * f64(S[0, 0]) + f64(S[0, 1]) * f64(S[0, 1])) + f64(S[0, 2]) * f64(S[0, 2])))
    inv = f32(1.0 / f64(scw))
    R, t = (S[:, :3] * inv).astype(f32), (S[:, 3] * inv).astype(f32)
    return R, t, -_rowdot(R.T.copy(), t, f32)


def _static(frame, src, opt, mutant, c):
    """what no round changes, per source: dict(reason, knife, knife_q, the taps, area = vIndices in the reference's order, hd = their
    Hamming distances, lvl_skip = SIM3's octave test of the inner loop, octs, er_skip = the right-image test of a mutant)"""
    mode = opt["mode"]
    reloc = mode == RELOC
    tgt = so._target(frame)
    ns = int(np.size(src["valid"]))
    R, t = np.asarray(frame["Rcw"], f32).reshape(3, 3), np.asarray(frame["tcw"], f32).reshape(3)
    K = np.asarray(frame["K"], f32).reshape(-1)
    Ow = np.asarray(frame["Ow"], f32).reshape(3)
    min_x, max_x, min_y, max_y = [f32(b) for b in frame["bounds"]]
    cols, rows, w_inv, h_inv = int(frame["grid"][0]), int(frame["grid"][1]), f32(frame["grid"][2]), f32(frame["grid"][3])
    sf, n_levels, log_scale = np.asarray(frame["scale_factors"], f32), int(np.size(frame["scale_factors"])), f32(frame["log_scale"])
    kx, ky = tgt["kp"][:, 0], tgt["kp"][:, 1]
    kr = np.asarray(frame.get("u_right", np.full(len(kx), -1.0)), f32).reshape(-1)
    octave, filed = tgt["octave"], tgt["ok"]
    c["unfiled"] += int((~filed).sum())
    th = f32(opt["th"])
    Xw_all, desc_all = np.asarray(src["Xw"], f32).reshape(-1, 3), np.asarray(src["desc"], np.uint8).reshape(-1, 32)
    half_open = (not reloc and mutant != "image_closed") or mutant == "image_half_open"
    reloc_order = (reloc and mutant != "reloc_invz_order") or mutant == "sim3_invz_order"
    recs = []
    for i in range(ns):
        rec = dict(reason=MATCHED, knife=[], knife_q=np.inf, proj_x=f32(0), proj_y=f32(0), level=0, area=np.zeros(0, np.int64),
                   hd=np.zeros(0, np.int64), lvl_skip=np.zeros(0, bool), octs=np.zeros(0, np.int64), er_skip=np.zeros(0, bool))
        recs.append(rec)
        if not src["valid"][i]:
            rec["reason"] = INVALID_SRC
            c["invalid"] += 1
            continue
        X, k = Xw_all[i], rec["knife"]
        with np.errstate(all="ignore"):
            p = _rowdot(R, X, f32) + t
            if reloc:
                invz = f32(1.0 / f64(p[2]))                        # :1502
                if mutant == "reloc_z_neg" and invz < 0:
                    rec["reason"] = Z_NEG
                    continue
            else:
                k.append(abs(float(p[2])) / max(float(np.linalg.norm(p.astype(f64))), 1e-30))
                if p[2] < f32(0.0):                                # :327
                    rec["reason"] = Z_NEG
                    c["z_neg"] += 1
                    continue
                if p[2] == 0 and np.signbit(p[2]):
                    c["z_minus_0"] += 1
                invz = f32(1.0) / p[2]
            if reloc_order:
                u, v = K[0] * p[0] * invz + K[2], K[1] * p[1] * invz + K[3]
            else:
                x, y = p[0] * invz, p[1] * invz
                u, v = K[0] * x + K[2], K[1] * y + K[3]
            k += [abs(float(u) - float(b)) / float(max_x - min_x) for b in (min_x, max_x)]
            k += [abs(float(v) - float(b)) / float(max_y - min_y) for b in (min_y, max_y)]
            if half_open:
                inside = u >= min_x and u < max_x and v >= min_y and v < max_y               # KeyFrame::IsInImage: a NaN fails
            else:
                inside = not (u < min_x or u > max_x or v < min_y or v > max_y)              # :1507-1510: a NaN passes
            if not inside:
                rec["reason"] = OUTSIDE
                c["outside"] += 1
                continue
            if np.isnan(u) or np.isnan(v):                         # the reference goes on to (int)floor(NaN); the library does not
                rec["reason"] = NONFINITE
                c["nonfinite"] += 1
                continue
            if reloc and p[2] < 0:
                c["z_neg_searched"] += 1
            PO = X - Ow
            d3 = f32(np.sqrt((f64(PO[0]) * f64(PO[0]) + f64(PO[1]) * f64(PO[1])) + f64(PO[2]) * f64(PO[2])))
            dmin, dmaxi = f32(src["dist_min_inv"][i]), f32(src["dist_max_inv"][i])
            k += [abs(float(d3) - float(dmin)) / float(dmin), abs(float(d3) - float(dmaxi)) / float(dmaxi)]
            if d3 < dmin or d3 > dmaxi:
                rec["reason"] = DISTANCE
                c["dist_near" if d3 < dmin else "dist_far"] += 1
                continue
            if not reloc:
                Pn = np.asarray(src["normal"], f32).reshape(-1, 3)[i]
                dot = (f64(PO[0]) * f64(Pn[0]) + f64(PO[1]) * f64(Pn[1])) + f64(PO[2]) * f64(Pn[2])
                k.append(abs(float(dot) - 0.5 * float(d3)) / float(d3))
                if (dot <= 0.5 * f64(d3)) if mutant == "angle_le" else (dot < 0.5 * f64(d3)):                # :354
                    rec["reason"] = ANGLE
                    c["angle"] += 1
                    continue
            ratio = f32(src["dist_max"][i]) / d3
            q = np.log(ratio) / log_scale                          # (numpy's float32 log stands in for logf)
            fl = np.ceil(q)
            if np.isnan(d3) or np.isnan(fl):
                rec["reason"] = NONFINITE
                c["nonfinite"] += 1
                continue
            rec["knife_q"] = min([abs(float(q) - e) for e in range(n_levels - 1)] + [np.inf])
            k.append(rec["knife_q"])
            level = 0 if fl < 0 else (n_levels - 1 if fl >= n_levels else int(fl))
            c["clamp_0" if fl < 0 else ("clamp_top" if fl >= n_levels else "level_mid")] += 1
            r = th * sf[level]
            top_plus1 = (reloc and mutant != "window_top_level") or mutant == "window_top_plus1"
            lvl_min, lvl_max = level - 1, level + (1 if top_plus1 else 0)
            a_x, b_x, a_y, b_y = ((u - min_x) - r) * w_inv, ((u - min_x) + r) * w_inv, ((v - min_y) - r) * h_inv, ((v - min_y) + r) * h_inv
            if np.isnan([a_x, b_x, a_y, b_y]).any():
                rec["reason"] = NONFINITE
                c["nonfinite"] += 1
                continue
            rec.update(proj_x=u, proj_y=v, level=level)
            big = lambda z: int(np.clip(z, -1e9, 1e9))
            min_cx, max_cx = max(0, big(np.floor(a_x))), min(cols - 1, big(np.ceil(b_x)))
            min_cy, max_cy = max(0, big(np.floor(a_y))), min(rows - 1, big(np.ceil(b_y)))
            if min_cx >= cols or max_cx < 0 or min_cy >= rows or max_cy < 0:
                rec["reason"] = EMPTY
                c["no_range"] += 1
                continue
            dx, dy = np.abs(kx - u), np.abs(ky - v)
            if filed.any():
                cx, cy = tgt["cx"][filed].astype(f64), tgt["cy"][filed].astype(f64)
                k += [float(np.min(np.abs(np.maximum(dx[filed], dy[filed]) - r) / r)),   # in the box: max(|dx|, |dy|) < r
                      float(np.min(np.abs(f64(a_x) - (cx + 1)))), float(np.min(np.abs(f64(b_x) - (cx - 1)))),
                      float(np.min(np.abs(f64(a_y) - (cy + 1)))), float(np.min(np.abs(f64(b_y) - (cy - 1))))]
            cells = [(ix, iy) for ix in range(min_cx, max_cx + 1) for iy in range(min_cy, max_cy + 1)]
            if mutant == "tie_cy_cx":
                cells = [(ix, iy) for iy in range(min_cy, max_cy + 1) for ix in range(min_cx, max_cx + 1)]
            area = []
            for ix, iy in cells:                                   # Frame:: / KeyFrame::GetFeaturesInArea
                for j in tgt["grid"][ix][iy]:
                    if reloc and (octave[j] < lvl_min or octave[j] > lvl_max):               # Frame.cc:398-405
                        c["level_out"] += 1
                        continue
                    if dx[j] < r and dy[j] < r:
                        area.append(j)
                    else:
                        c["box_out"] += 1
            area = np.array(area, np.int64)
            if len(area) == 0:
                rec["reason"] = EMPTY
                c["area_empty"] += 1
                continue
            octs = octave[area]
            ur = u - (K[4] if len(K) > 4 else f32(0)) * invz
            rec.update(area=area, octs=octs, hd=so.popcount_rows(tgt["desc"][area], desc_all[i]),
                       lvl_skip=(octs < lvl_min) | (octs > lvl_max) if not reloc else np.zeros(len(area), bool),
                       er_skip=(kr[area] > 0) & (np.abs(ur - kr[area]) > r) if mutant == "right_test" else np.zeros(len(area), bool))
    return recs


def _pick(rec, blocked, opt, mutant, c):
    """the inner loop and the keep rule for one source: (choice, dist, reason)"""
    if rec["reason"] != MATCHED:
        return -1, -1, rec["reason"]
    best_dist, best_idx, best_dist2, best_level, best_level2 = 256, -1, 256, -1, -1
    for n, idx in enumerate(rec["area"]):
        why = blocked(int(idx))
        if why:                                                    # :1541 / :375
            c[why] += 1
            continue
        if rec["lvl_skip"][n]:                                     # :380
            c["octave_skip"] += 1
            continue
        if rec["er_skip"][n]:
            continue
        d = int(rec["hd"][n])
        if d < best_dist:
            best_dist2, best_level2 = best_dist, best_level
            best_dist, best_idx, best_level = d, int(idx), int(rec["octs"][n])
            c["best_update"] += 1
        else:
            if d < best_dist2:
                best_dist2, best_level2 = d, int(rec["octs"][n])
            c["no_update"] += 1
    if best_idx < 0:
        c["none_eligible"] += 1
        return -1, -1, NONE_ELIGIBLE
    limit = 100 if mutant == "accept_100" else int(opt["orb_dist"])
    if (best_dist >= limit) if mutant == "accept_lt" else (best_dist > limit):
        c["above_th"] += 1
        return -1, best_dist, ABOVE_TH
    if mutant == "ratio_test" and best_level == best_level2 and f32(best_dist) > f32(0.8) * f32(best_dist2):
        return -1, best_dist, po.RATIO
    c["kept"] += 1
    return best_idx, best_dist, MATCHED


def _action(frame, src, opt, choice, c):
    """the writes of the loop in source order and the tail :1577-1596: (slot_src, n_matches, bin, hist, ind)"""
    ns, n = len(choice), int(np.size(frame["octave"]))
    ori = opt["mode"] == RELOC and opt["check_orientation"]
    slot_src, n_matches = np.full(n, -1, np.int64), 0
    bins, hist, ind = np.full(ns, -1, np.int64), np.zeros(HISTO_LENGTH, np.int64), [-1, -1, -1]
    for i in range(ns):
        s = int(choice[i])
        if s < 0:
            continue
        slot_src[s] = i
        n_matches += 1
        if ori:
            bins[i] = rot_bin(src["angle"][i], frame["kp_angle"][s], c)
            if bins[i] < 0:
                c["bin_invalid"] += 1
            else:
                hist[bins[i]] += 1
    if ori:
        ind = three_maxima(hist)
        c["maxima"] += 1
        for i in range(ns):
            if bins[i] >= 0 and bins[i] not in ind:
                slot_src[int(choice[i])] = -2
                n_matches -= 1
                c["nulled"] += 1
    elif opt["mode"] == RELOC:
        c["ori_off"] += 1
    return slot_src, n_matches, bins, hist, np.array(ind, np.int64)


def _result(recs, picks, action, counters, extra):
    out = dict(choice=np.array([p[0] for p in picks], np.int64), dist=np.array([p[1] for p in picks], np.int64),
               reason=np.array([p[2] for p in picks], np.int64), proj_x=np.array([r["proj_x"] for r in recs], f32),
               proj_y=np.array([r["proj_y"] for r in recs], f32), level=np.array([r["level"] for r in recs], np.int64),
               knife_q=np.array([r["knife_q"] for r in recs], f64),
               knife=np.array([min(r["knife"]) if r["knife"] else np.inf for r in recs], f64), counters=counters)
    out["slot_src"], out["n_matches"], out["bin"], out["hist"], out["ind"] = action
    out.update(extra)
    return {k: (v.reshape(-1) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def _counters(mode):
    return collections.Counter({b: 0 for b in BRANCHES[mode]})


def serial(frame, src, opt, mutant=None):
    """the reference's loop: the sources in order over the live slot table"""
    assert mutant is None or mutant in MUTANTS
    c = _counters(opt["mode"])
    recs = _static(frame, src, opt, mutant, c)
    n = int(np.size(frame["octave"]))
    holder = [("blocked_initial" if b else "") for b in np.asarray(frame["slot_blocked"]).reshape(-1)[:n]]
    picks = []
    for i, rec in enumerate(recs):
        p = _pick(rec, lambda idx: holder[idx], opt, mutant, c)
        picks.append(p)
        if p[0] >= 0:                                              # the slot now holds THIS point: non-null
            holder[p[0]] = "" if (mutant == "non_blocking" and not src["blocks"][i]) else "blocked_by_source"
    choice = [p[0] for p in picks]
    return _result(recs, picks, _action(frame, src, opt, choice, c), c, {})


def rounds(frame, src, opt):
    """the parallel iteration of csrc/search_projection.hpp in numpy with every source blocking; n_rounds as the library counts them"""
    c = _counters(opt["mode"])
    recs = _static(frame, src, opt, None, c)
    ns, n = len(recs), int(np.size(frame["octave"]))
    initial = np.asarray(frame["slot_blocked"]).reshape(-1)[:n].astype(bool)
    NO_CLAIM = 1 << 31
    claim, prev, n_rounds = np.full(n, NO_CLAIM, np.int64), [-1] * ns, 0
    while True:
        assert n_rounds <= ns, "the rounds did not reach their fixed point"
        picks = [_pick(rec, lambda idx, i=i: "blocked_initial" if initial[idx] else ("blocked_by_source" if claim[idx] < i else ""), opt, None, c)
                 for i, rec in enumerate(recs)]
        choice = [p[0] for p in picks]
        n_rounds += 1
        claim = np.full(n, NO_CLAIM, np.int64)
        for i in range(ns):
            if choice[i] >= 0:
                claim[choice[i]] = min(claim[choice[i]], i)
        if choice == prev:
            break
        prev = choice
    return _result(recs, picks, _action(frame, src, opt, choice, _counters(opt["mode"])), c, dict(n_rounds=n_rounds))


def differs(a, b):
    """per source: any output differs (floats by bits)"""
    d = np.zeros(len(a["choice"]), bool)
    for k in PER_SOURCE:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        d |= (x.view(np.uint32) != y.view(np.uint32)) if x.dtype == np.float32 else (x.astype(np.int64) != y.astype(np.int64))
    return d


def n_differing(g, r):
    """sources with any differing output + slots with a differing holder + differing scalars of the call"""
    return (int(differs(g, r).sum()) + int((np.asarray(g["slot_src"], np.int64) != np.asarray(r["slot_src"], np.int64)).sum())
            + int(int(g["n_matches"]) != int(r["n_matches"])) + int((np.asarray(g["hist"], np.int64) != np.asarray(r["hist"], np.int64)).sum())
            + int(list(g["ind"]) != list(r["ind"])))


# ---- the hand-made scene of tests/search_projection_oracle.py: every value chosen so that float32 arithmetic is exact ----------------
# identity pose with signed zeros, fx = fy = 512, z = 4: u = 128 * X + 320 exactly in both orders of operations.  5 levels at 1.5; th =
# 3: radius 3 * 1.5^level (level 1: 4.5).  Every case sits in a box of its own, 100 x 40 pixels.
E_TH = 3.0
E_LEVELS = po.E_LEVELS
OPT = {RELOC: dict(mode=RELOC, th=E_TH, orb_dist=100, check_orientation=True), SIM3: dict(mode=SIM3, th=E_TH, orb_dist=TH_LOW, check_orientation=False)}


class Builder(po.Builder):
    def __init__(self, mode, seed):
        po.Builder.__init__(self, po.LAST, seed)
        self.kf_mode = mode
        self.radius = lambda level: f32(E_TH * float(po.E_SF[level]))

    def set_angle(self, kp, angle):
        self.kps[kp] = self.kps[kp][:5] + (f32(angle),)

    def finish(self, name, **opt):
        f = po.Builder.finish(self, name)
        f["opt"] = dict(OPT[self.kf_mode], **opt)
        return f


@functools.lru_cache(maxsize=None)
def contention_scene(mode, only=None):
    """the contention cases of one mode (`only`: one group alone); cases[name] = dict(src=[...], kp=[...], want...)"""
    b = Builder(mode, 8100 + mode)
    L = 1
    want = lambda name: only is None or only == name
    if want("pair"):                     # two sources want one key point: the later takes its second choice.  The first one's point has
        c = b.box()                      # no observations (blocks = 0): it blocks all the same
        D, s, k = _spread(b, c, L, (4, 8), first=0)
        srcs = [b.src(_at(c, s, 1), D, L, blocks=False), b.src(_at(c, s, 1), D, L)]
        b.cases["pair"] = dict(src=srcs, kp=k, choice=[k[0], k[1]])
    if want("chain"):                    # source k prefers key point k - 1 and falls back to k: 6 rounds
        c = b.box()
        D, s, k = _spread(b, c, L, (4, 8, 16, 32, 48), first=0)
        srcs = [b.src(_at(c, s, 0.5), D, L)] + [b.src(_at(c, s, m), D, L) for m in range(1, 5)]
        b.cases["chain"] = dict(src=srcs, kp=k, choice=list(k), n_rounds=6)
    if want("blocked_initially"):        # the best slot held a point before the call
        c = b.box()
        D, s, k = _spread(b, c, L, (4,), first=0, blocked=True)
        k.append(b.kp((c[0] - 40.0 + 0.5 * s, c[1] + 1.0), L - 1, b.flip(D, 9)))
        srcs = [b.src(_at(c, s, 0.5), D, L)]
        b.cases["blocked_initially"] = dict(src=srcs, kp=k, choice=[k[1]])
    if want("listed_twice"):             # the same point twice in the list: the second copy takes the second best
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 3)), b.kp((c[0] - 0.5, c[1] - 0.5), L, b.flip(D, 12))]
        srcs = [b.src(c, D, L), b.src(c, D, L)]
        b.cases["listed_twice"] = dict(src=srcs, kp=k, choice=[k[0], k[1]], dist=[3, 12])
    if mode == RELOC and want("ori"):    # 8 plain matches in bin 0, 4 in bin 12, 3 in bin 6, and one alone in bin 3: removed
        for m in range(15):
            c = b.box()
            D, s, k = _spread(b, c, L, (3 + m % 5,), first=0)
            b.src(_at(c, s, 0.5), D, L, angle=(200.0 if m >= 12 else 10.0 + m))
            b.set_angle(k[0], 20.0 if m >= 12 else 10.0 + m + (5.0 if m % 3 == 0 else -5.0))
        c = b.box()
        D, s, k = _spread(b, c, L, (4,), first=0)
        srcs = [b.src(_at(c, s, 0.5), D, L, angle=90.0)]
        b.cases["hist_removed"] = dict(src=srcs, kp=k, choice=[k[0]], slot_src={k[0]: -2}, bin=[3])
        for name, a_src, a_kp, want_bin in (("bin_wrap", 900.0, 0.0, 0), ("bin_31", 930.0, 0.0, -1), ("bin_nan", np.nan, 0.0, -1), ("rot_neg", 5.0, 355.0, 0)):
            c = b.box()
            D, s, k = _spread(b, c, L, (5,), first=0)
            b.set_angle(k[0], a_kp)
            srcs = [b.src(_at(c, s, 0.5), D, L, angle=a_src)]
            b.cases[name] = dict(src=srcs, kp=k, choice=[k[0]], bin=[want_bin], slot_src={k[0]: srcs[0]})
    return b.finish("contention" if only is None else only)


@functools.lru_cache(maxsize=None)
def edge_scene(mode, orb_dist):
    """ties, the exact thresholds of both modes, the octave windows, the refusals and the cases where the reference is undefined"""
    b = Builder(mode, 8200 + mode)
    reloc = mode == RELOC
    L = 1
    R = float(b.radius(L))
    # ties across cell x, cell y and index: the LOWER index lies later in the traversal; tie_diag: cell x and cell y disagree
    for name, off_a, off_b, first in (("tie_cx", (1.0, 1.5), (-1.0, 1.5), 1), ("tie_cy", (1.5, 1.0), (1.0, -1.0), 1), ("tie_cell", (1.0, 1.0), (2.0, 2.0), 0),
                                      ("tie_diag", (1.0, -1.0), (-1.0, 1.0), 1)):
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + off_a[0], c[1] + off_a[1]), L, b.flip(D, 7)), b.kp((c[0] + off_b[0], c[1] + off_b[1]), L - 1, b.flip(D, 7))]
        b.cases[name] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[first]], dist=[7])
    # best and second at one level, 40 > 0.8 * 45: no ratio test here
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 1.0, c[1] + 1.0), L, b.flip(D, 40)), b.kp((c[0] + 2.0, c[1] + 2.0), L, b.flip(D, 45))]
    b.cases["no_ratio"] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[0]], dist=[40])
    # the accept threshold
    for name, h in (("dist_at_th", orb_dist), ("dist_above_th", orb_dist + 1)):
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] - 0.25), L, b.flip(D, h))]
        b.cases[name] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[0] if h == orb_dist else -1], dist=[h], reason=[MATCHED if h == orb_dist else ABOVE_TH])
    # |dx| == radius exactly: outside the strict box; one float32 step nearer: inside
    for name, hit in (("dx_eq_r", False), ("dx_below_r", True)):
        c = b.box()
        D = b.desc()
        kx = f32(c[0] + R) if not hit else _next(c[0] + R, False)
        assert (abs(kx - f32(c[0])) == f32(R)) != hit
        k = [b.kp((kx, c[1]), L, D.copy())]
        si = b.src(c, D, L)
        b.cases[name] = dict(src=[si], kp=k, choice=[k[0] if hit else -1], reason=[MATCHED if hit else EMPTY])
        b.exact.add(si)
    # a key point with u_right > 0 far from the projection still matches: no right-image test
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 3), u_right=c[0] + 60.0)]
    b.cases["right_far"] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[0]], dist=[3])
    # u == max_x: inside the closed test (RELOC), outside the half-open one (SIM3); one float32 step below: inside in both
    for name, X0, inside in (("u_eq_max", 2.5, reloc), ("u_below_max", 2.5 - 2.0 ** -21, True)):
        si = b.src((640.0, 200.0), b.desc(), L, X=(X0, (200.0 - 240.0) / 128.0, po.E_Z))
        b.cases[name] = dict(src=[si], reason=[EMPTY if inside else OUTSIDE], proj_x=(f32(640.0) if name == "u_eq_max" else _next(640.0, False)) if inside else f32(0))
        b.exact.add(si)
    for name, Y0, inside in (("v_eq_max", 1.875, reloc),):
        si = b.src((100.0, 480.0), b.desc(), L, X=((100.0 - 320.0) / 128.0, Y0, po.E_Z))
        b.cases[name] = dict(src=[si], reason=[EMPTY if inside else OUTSIDE])
        b.exact.add(si)
    si = b.src((0.0, 300.0), b.desc(), L)
    b.cases["u_eq_min"] = dict(src=[si], reason=[EMPTY])
    b.exact.add(si)
    # the sign of z.  RELOC has no test: z = -4 projects where z = +4 does and matches; z == +-0.0 gives an infinite u (outside);
    # with x == 0 too, u = 0 * inf is NaN, which passes every compare of RELOC and fails IsInImage in SIM3
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 6))]
    si = b.src(c, D, L, z=-po.E_Z)
    b.cases["z_negative"] = dict(src=[si], kp=k, choice=[k[0] if reloc else -1], reason=[MATCHED if reloc else Z_NEG])
    for name, X, why in (("z_plus_0", (0.5, 0.5, 0.0), OUTSIDE), ("z_minus_0", (0.5, 0.5, -0.0), OUTSIDE),
                         ("z_0_x_0", (0.0, 0.0, 0.0), NONFINITE if reloc else OUTSIDE), ("x_nan", (np.nan, 0.0, 4.0), NONFINITE if reloc else OUTSIDE),
                         ("z_tiny_neg", (0.5, 0.5, -float(np.finfo(f32).tiny)), OUTSIDE if reloc else Z_NEG)):
        si = b.src(None, b.desc(), L, X=X, normal=(0.0, 0.0, 1.0))
        b.cases[name] = dict(src=[si], reason=[why])
        b.exact.add(si)
    si = b.src(b.box(), b.desc(), L, valid=False)
    b.cases["invalid"] = dict(src=[si], reason=[INVALID_SRC])
    si = b.src(None, b.desc(), L, X=((-300.0 - 320.0) / 128.0, 0.0, po.E_Z))
    b.cases["u_below_min"] = dict(src=[si], reason=[OUTSIDE])
    si = b.src(None, b.desc(), L, X=(0.0, (-5.0 - 240.0) / 128.0, po.E_Z))
    b.cases["v_below_min"] = dict(src=[si], reason=[OUTSIDE])
    si = b.src(b.box(), b.desc(), L)
    b.cases["empty_box"] = dict(src=[si], reason=[EMPTY])
    # a key point never filed (round(636 / 10) == 64 == grid_cols) with the perfect descriptor next to a filed one
    D = b.desc()
    si = b.src(None, D, L, X=((633.0 - 320.0) / 128.0, (100.0 - 240.0) / 128.0, po.E_Z))
    k = [b.kp((636.0, 100.0), L, D.copy()), b.kp((632.0, 100.5), L, b.flip(D, 30))]
    b.cases["unfiled"] = dict(src=[si], kp=k, choice=[k[1]], dist=[30])
    # the distance limits: equal passes, one step inside refuses
    for name, which, step, ok in (("dist_eq_min_inv", "dist_min_inv", 0, True), ("dist_eq_max_inv", "dist_max_inv", 0, True),
                                  ("dist_below_min_inv", "dist_min_inv", 1, False), ("dist_above_max_inv", "dist_max_inv", -1, False)):
        c = b.box()
        D = b.desc()
        si = b.src(c, D, L)
        X = b.srcs[si]["Xw"]
        d3 = f32(np.sqrt((f64(X[0]) * f64(X[0]) + f64(X[1]) * f64(X[1])) + f64(X[2]) * f64(X[2])))
        b.srcs[si][which] = d3 if step == 0 else _next(d3, step > 0)
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 3))]
        b.cases[name] = dict(src=[si], kp=k, choice=[k[0] if ok else -1], reason=[MATCHED if ok else DISTANCE])
        b.exact.add(si)
    # the angle test of SIM3: on the axis PO = (0, 0, 4) and the normal (., 0, c) give PO.Pn = 4 c exactly against 0.5 * dist = 2.  RELOC
    # has no such test: its second source finds the slot taken
    D = b.desc()
    k = [b.kp((321.0, 240.5), L, b.flip(D, 2))]
    srcs = [b.src((320.0, 240.0), D, L, normal=(np.sqrt(1.0 - float(cz) ** 2), 0.0, cz)) for cz in (f32(0.5), _next(0.5, False))]
    b.cases["angle_eq"] = dict(src=srcs[:1], kp=k, choice=[k[0]], reason=[MATCHED])
    b.cases["angle_below"] = dict(src=srcs[1:], kp=k, choice=[-1], reason=[NONE_ELIGIBLE if reloc else ANGLE])
    b.exact.update(srcs)
    si = b.src((320.0, 200.0), b.desc(), L)
    b.srcs[si]["dist_max"] = f32(np.nan)
    b.cases["dist_max_nan"] = dict(src=[si], reason=[NONFINITE])
    b.exact.add(si)
    # the level clamped at 0 and at the top: the window is the CLAMPED level's; perfect descriptors wait two levels outside it
    for name, q, lvl in (("clamp_0", -2.6, 0), ("clamp_top", 7.3, E_LEVELS - 1)):
        c = b.box()
        D = b.desc()
        si = b.src(c, D, 0, q_off=q)
        b.srcs[si]["dist_min_inv"], b.srcs[si]["dist_max_inv"] = f32(0.01), f32(1000.0)
        k = [b.kp((c[0] + 0.5, c[1] - 0.5), lvl, b.flip(D, 9)), b.kp((c[0] - 0.5, c[1] + 0.5), 2, D.copy())]
        b.cases[name] = dict(src=[si], kp=k, choice=[k[0]], dist=[9], level=[lvl])
    # the octave window around level 2: level + 1 is inside in RELOC only; level + 2 and level - 2 in neither
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 0.5, c[1] + 0.5), 2, b.flip(D, 11)), b.kp((c[0] - 0.5, c[1] - 0.5), 3, b.flip(D, 1))]
    b.cases["octave_level_plus_1"] = dict(src=[b.src(c, D, 2)], kp=k, choice=[k[1] if reloc else k[0]], dist=[1 if reloc else 11])
    for name, o in (("octave_level_plus_2", 4), ("octave_level_minus_2", 0)):
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), 2, b.flip(D, 11)), b.kp((c[0] - 0.5, c[1] - 0.5), o, D.copy())]
        b.cases[name] = dict(src=[b.src(c, D, 2)], kp=k, choice=[k[0]], dist=[11])
    # only key points outside the window: RELOC's area is empty, SIM3 found them in the area and skipped them
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 0.5, c[1] + 0.5), 4, D.copy())]
    b.cases["octave_only_outside"] = dict(src=[b.src(c, D, 2)], kp=k, choice=[-1], reason=[EMPTY if reloc else NONE_ELIGIBLE])
    return b.finish("edges", orb_dist=orb_dist)


def with_scw(f, name, s):
    """the fixture with the pose given as Scw = s [Rcw | tcw] and decomposed again"""
    fr = f["frame"]
    S = np.concatenate([f32(s) * np.asarray(fr["Rcw"], f32).reshape(3, 3), (f32(s) * np.asarray(fr["tcw"], f32)).reshape(3, 1)], 1).astype(f32)
    R, t, Ow = decompose_scw(S)
    return dict(f, name=name, frame=dict(fr, Scw=S, Rcw=R, tcw=t, Ow=Ow))


def random_scene(mode, spec_index=0, n=None, seed=0, th=10.0, orb_dist=None, scale=None):
    """the random frames and pool of tests/search_projection_oracle.py (a fifth of the slots taken at entry, a tenth of the sources
    invalid) under one of the two modes; `scale`: the pose handed over as a Sim3 of that scale"""
    f = po.random_scene(po.LOCAL, spec_index, n=n, seed=seed)
    opt = dict(OPT[mode], th=th, orb_dist=OPT[mode]["orb_dist"] if orb_dist is None else orb_dist)
    f = dict(f, opt=opt)
    return f if scale is None else with_scw(f, f["name"], scale)


STRIDE_N = (0, 1, 63, 64, 65, 4096, 4097)
RANDOM_SEED = {RELOC: (0, 0, 5), SIM3: (0, 0, 5)}


@functools.lru_cache(maxsize=None)
def fixtures(mode):
    """name -> dict(frame, src, opt, cases, exact); treat as read-only"""
    out = dict(contention=contention_scene(mode), chain=contention_scene(mode, "chain"), edges=edge_scene(mode, OPT[mode]["orb_dist"]))
    variant = lambda f, name, **o: dict(f, name=name, opt=dict(f["opt"], **o), cases={} if o else f["cases"])
    if mode == RELOC:
        out["edges_64"] = dict(edge_scene(mode, 64), name="edges_64")
        out["contention_no_ori"] = variant(out["contention"], "contention_no_ori", check_orientation=False)
    else:
        out["scale_half"] = with_scw(out["edges"], "scale_half", 0.5)
        out["scale_two"] = with_scw(out["edges"], "scale_two", 2.0)
    # a grid that covers only the left half of the image (cells of 5 pixels): sources beyond it have no cell range at all
    out["edges_half_grid"] = dict(out["edges"], name="edges_half_grid", cases={}, frame=dict(out["edges"]["frame"], grid=(64, 48, f32(0.2), f32(0.2))))
    for s in range(3):
        out["random_%d" % s] = random_scene(mode, s, seed=RANDOM_SEED[mode][s], scale=(None, 0.75, 1.3)[s] if mode == SIM3 else None)
    out["random_th3"] = random_scene(mode, 0, th=3.0, orb_dist=64 if mode == RELOC else None)
    for kk, n in enumerate(STRIDE_N):
        out["stride_%d" % n] = random_scene(mode, 0, n=n, seed=10 + kk)
    return out


@functools.lru_cache(maxsize=None)
def result(mode, name, mutant=None):
    f = fixtures(mode)[name]
    return serial(f["frame"], f["src"], f["opt"], mutant)


@functools.lru_cache(maxsize=None)
def result_rounds(mode, name):
    f = fixtures(mode)[name]
    return rounds(f["frame"], f["src"], f["opt"])


take_sources = po.take_sources


def weave(f):
    """the fixture with unrelated gated-out sources woven in (an invalid one, one far outside the image to the left, one far outside
    to the right, in turn, before every source).  Returns (fixture, positions of the original sources)"""
    src, ns = f["src"], int(np.size(f["src"]["valid"]))
    extra = {k: v.copy() for k, v in take_sources(src, np.arange(ns) % max(ns, 1)).items()}
    R, t = np.asarray(f["frame"]["Rcw"], f64).reshape(3, 3), np.asarray(f["frame"]["tcw"], f64).reshape(3)
    for i in range(ns):
        if i % 3 == 0:
            extra["valid"][i] = 0
        else:
            Y = np.array((-40.0, 0.2, 4.0)) if i % 3 == 1 else np.array((40.0, 0.1, 4.0))
            extra["Xw"][i] = (R.T @ (Y - t)).astype(f32)
            extra["valid"][i] = 1
    woven = {k: np.stack([extra[k], np.asarray(src[k])], 1).reshape((2 * ns,) + np.asarray(src[k]).shape[1:]) for k in src}
    return dict(f, src=woven), np.arange(ns) * 2 + 1
