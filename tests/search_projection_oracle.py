"""A line-by-line SERIAL restatement in np.float32 of the tracking thread's projection searches -- LOCAL: Frame::isInFrustum (reference
src/Frame.cc:306-362) and ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:45-129); LAST:
ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (:1328-1470) -- with Frame::GetFeaturesInArea,
Frame::PosInGrid, MapPoint::PredictScale and ComputeThreeMaxima: the yardstick of qsp_search_by_projection, and the fixtures its
tests share.  Written here from the formulas; helpers of tests/search_sim3_oracle.py and scenes of tests/fuse_oracle.py are used.

serial() walks the sources in order over a live slot table, as the reference does: a slot is skipped when the point it holds has
observations -- at entry frame["slot_blocked"], afterwards src["blocks"] of the last source written there.  rounds() is a numpy
version of the parallel iteration of csrc/search_projection.hpp (claim[idx] = the smallest blocking source that chose idx in the
round before; source i is blocked where claim[idx] < i) and returns its round count.  Both share the per-source part that no
round changes (projection, gates, area) and the `<` / `else if <` best-and-second loop.

The arithmetic: cv::Mat products are row sums in double rounded to float32 once with t added in float32; LOCAL 1.0f / PcZ and LAST
(float)(1.0 / z); u = fx * x * invz + cx left to right; PO = P - Ow in float32, cv::norm(PO) and PO.dot(Pn) summed in double; viewCos =
(float)(dot / dist); compares against double literals in double; numpy's float32 log stands in for logf.

serial() counts every branch it takes (BRANCHES) and returns per source the KNIFE-EDGE DISTANCE, the smallest relative distance of
any float decision to its threshold: |z| / |p|; u, v against the four bounds (relative to the extent); dist against both limits;
viewCos against the limit and against 0.998; log(ratio) / log_scale against the integers at which the clamped level changes; for
the filed key points ||dx| - r| / r, ||dy| - r| / r and the ends of the cell range; |er - radius| / radius of the stereo key
points of the area; |d1 - nn_ratio * d2| / d1 where the ratio test is decided.  The only operation in which the device and numpy
may differ is logf (a few float32 ulp: under 1e-5 levels at these ratios); everything else is one IEEE operation at a time on
both sides and has the same bits.  So the level decision (knife_q) must keep THRESHOLD = 1e-4 levels from every integer, and no
source other than the deliberately exact ones may sit ON any threshold: its knife-edge distance stays above ON_THRESHOLD = 1e-6,
about eight float32 steps.

`mutant` makes ONE deliberate mistake (MUTANTS); tests/test_oracle_search_projection.py shows that each changes an output."""
import collections
import functools
import os

import numpy as np

from tests import fuse_oracle as fo
from tests import search_sim3_oracle as so
from tests.search_sim3_oracle import _flip, _rowdot, f32, f64

LOCAL, LAST = 0, 1
TH_HIGH, HISTO_LENGTH = 100, 30
MATCHED, INVALID_SRC, Z_NEG, OUTSIDE, DISTANCE, ANGLE, NONFINITE, EMPTY, NONE_ELIGIBLE, ABOVE_TH, RATIO = range(11)
REASONS = ("matched", "invalid", "z_neg", "outside", "distance", "angle", "nonfinite", "empty", "none_eligible", "above_th", "ratio")
MUTANTS = ("ignore_src_blocks", "all_block", "best_le", "level_window_wide", "half_open_image", "er_no_scale", "ratio_no_level",
           "first_writer", "null_skip_overwritten")
MUTANTS_OF = {0: MUTANTS[:8], 1: tuple(m for m in MUTANTS if m not in ("level_window_wide", "ratio_no_level"))}   # by mode: what it has
THRESHOLD, ON_THRESHOLD = 1e-4, 1e-6
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "search_projection_margins.json")
PER_SOURCE = ("choice", "dist", "reason", "dist2", "level_best", "level2", "in_view", "proj_x", "proj_y", "proj_xr", "level", "view_cos", "bin")
BRANCHES = {
    LOCAL: ("invalid", "z_neg", "outside_u", "outside_v", "nonfinite", "dist_near", "dist_far", "angle", "clamp_0", "clamp_top", "level_mid",
            "r_25", "r_40", "th_factor", "th_one", "no_range", "area_empty", "blocked_initial", "blocked_by_source", "er_skip", "er_pass",
            "kp_mono", "best_update", "second_demoted", "second_update", "no_update", "none_eligible", "above_th", "ratio_refused",
            "ratio_level_differs", "kept", "overwrite", "level_out", "box_out", "unfiled"),
    LAST: ("invalid", "z_neg", "outside_u", "outside_v", "nonfinite", "forward", "forward_octave_0", "backward", "neither", "mono", "no_range",
           "area_empty", "blocked_initial", "blocked_by_source", "er_skip", "er_pass", "kp_mono", "best_update", "no_update", "none_eligible",
           "above_th", "kept", "overwrite", "level_out", "box_out", "unfiled", "rot_neg", "bin_wrap", "bin_invalid", "nulled",
           "nulled_overwritten", "maxima_3", "maxima_cut"),
}


def rot_bin(a_src, a_tgt, c=None):
    """:1433-1439 in float32; -1 where the reference's assert would fire (counted in no bin)"""
    with np.errstate(all="ignore"):
        rot = f32(a_src) - f32(a_tgt)
        if rot < 0.0:
            rot = rot + f32(360.0)
            if c is not None:
                c["rot_neg"] += 1
        v = f64(rot * (f32(1.0) / f32(HISTO_LENGTH)))
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)                 # round(): half away from zero
    if not (r >= 0 and r <= HISTO_LENGTH):
        return -1
    if int(r) == HISTO_LENGTH and c is not None:
        c["bin_wrap"] += 1
    return 0 if int(r) == HISTO_LENGTH else int(r)


def three_maxima(hist):
    """ComputeThreeMaxima (:1601-1642) on the bin counts"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        s = int(s)
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        i2 = i3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        i3 = -1
    return [i1, i2, i3]


def tlc_z(frame, opt):
    """:1341-1346: the third component of Rlw * (-Rcw^T tcw) + tlw"""
    R, t = np.asarray(frame["Rcw"], f32).reshape(3, 3), np.asarray(frame["tcw"], f32).reshape(3)
    twc = -_rowdot(R.T.copy(), t, f32)
    Rl, tl = np.asarray(opt["last_Rcw"], f32).reshape(3, 3), np.asarray(opt["last_tcw"], f32).reshape(3)
    return (_rowdot(Rl, twc, f32) + tl)[2]


def _static(frame, src, opt, mutant, c):
    """what no round changes, per source: dict(reason, knife, the isInFrustum outputs, area = vIndices in the reference's order,
    hd = their Hamming distances, er_skip = the stereo test, octs)"""
    mode = opt["mode"]
    tgt = so._target(frame)
    ns = int(np.size(src["valid"]))
    R, t = np.asarray(frame["Rcw"], f32).reshape(3, 3), np.asarray(frame["tcw"], f32).reshape(3)
    K = np.asarray(frame["K"], f32).reshape(5)
    min_x, max_x, min_y, max_y = [f32(b) for b in frame["bounds"]]
    cols, rows, w_inv, h_inv = int(frame["grid"][0]), int(frame["grid"][1]), f32(frame["grid"][2]), f32(frame["grid"][3])
    sf, n_levels, log_scale = np.asarray(frame["scale_factors"], f32), int(np.size(frame["scale_factors"])), f32(frame["log_scale"])
    kx, ky, kr = tgt["kp"][:, 0], tgt["kp"][:, 1], np.asarray(frame["u_right"], f32).reshape(-1)
    octave, filed = tgt["octave"], tgt["ok"]
    c["unfiled"] += int((~filed).sum())
    th = f32(opt["th"])
    Xw_all, desc_all = np.asarray(src["Xw"], f32).reshape(-1, 3), np.asarray(src["desc"], np.uint8).reshape(-1, 32)
    if mode == LAST:
        tz = tlc_z(frame, opt)
        forward = bool(tz > f32(frame["mb"])) and not opt["mono"]
        backward = bool(-tz > f32(frame["mb"])) and not opt["mono"]
        c["mono"] += int(bool(opt["mono"]))
    recs = []
    for i in range(ns):
        rec = dict(reason=MATCHED, knife=[], knife_q=np.inf, in_view=0, proj_x=f32(0), proj_y=f32(0), proj_xr=f32(0), level=0, view_cos=f32(0),
                   area=np.zeros(0, np.int64), hd=np.zeros(0, np.int64), er_skip=np.zeros(0, bool), octs=np.zeros(0, np.int64))
        recs.append(rec)
        if not src["valid"][i]:
            rec["reason"] = INVALID_SRC
            c["invalid"] += 1
            continue
        X, k = Xw_all[i], rec["knife"]
        with np.errstate(all="ignore"):
            p = _rowdot(R, X, f32) + t
            k.append(abs(float(p[2])) / max(float(np.linalg.norm(p.astype(f64))), 1e-30))
            if mode == LOCAL:
                if p[2] < f32(0.0):                                # Frame.cc:320
                    rec["reason"] = Z_NEG
                    c["z_neg"] += 1
                    continue
                invz = f32(1.0) / p[2]
            else:
                invz = f32(1.0 / f64(p[2]))                        # :1365
                if invz < 0:
                    rec["reason"] = Z_NEG
                    c["z_neg"] += 1
                    continue
            u, v = K[0] * p[0] * invz + K[2], K[1] * p[1] * invz + K[3]
            ur = u - K[4] * invz
            k += [abs(float(u) - float(b)) / float(max_x - min_x) for b in (min_x, max_x)]
            k += [abs(float(v) - float(b)) / float(max_y - min_y) for b in (min_y, max_y)]
            if u < min_x or (u >= max_x if mutant == "half_open_image" else u > max_x):
                rec["reason"] = OUTSIDE
                c["outside_u"] += 1
                continue
            if v < min_y or (v >= max_y if mutant == "half_open_image" else v > max_y):
                rec["reason"] = OUTSIDE
                c["outside_v"] += 1
                continue
            if np.isnan(u) or np.isnan(v):                         # the reference goes on to (int)floor(NaN); the library does not
                rec["reason"] = NONFINITE
                c["nonfinite"] += 1
                continue
            if mode == LOCAL:
                PO = X - np.asarray(frame["Ow"], f32).reshape(3)
                d3 = f32(np.sqrt((f64(PO[0]) * f64(PO[0]) + f64(PO[1]) * f64(PO[1])) + f64(PO[2]) * f64(PO[2])))
                Pn = np.asarray(src["normal"], f32).reshape(-1, 3)[i]
                dot = (f64(PO[0]) * f64(Pn[0]) + f64(PO[1]) * f64(Pn[1])) + f64(PO[2]) * f64(Pn[2])
                view_cos = f32(dot / f64(d3))
                dmin, dmaxi = f32(src["dist_min_inv"][i]), f32(src["dist_max_inv"][i])
                k += [abs(float(d3) - float(dmin)) / float(dmin), abs(float(d3) - float(dmaxi)) / float(dmaxi)]
                if d3 < dmin or d3 > dmaxi:
                    rec["reason"] = DISTANCE
                    c["dist_near" if d3 < dmin else "dist_far"] += 1
                    continue
                k.append(abs(float(view_cos) - float(f32(opt["view_cos_limit"]))))
                if view_cos < f32(opt["view_cos_limit"]):
                    rec["reason"] = ANGLE
                    c["angle"] += 1
                    continue
                ratio = f32(src["dist_max"][i]) / d3
                q = np.log(ratio) / log_scale                      # (numpy's float32 log stands in for logf)
                fl = np.ceil(q)
                if np.isnan(d3) or np.isnan(view_cos) or np.isnan(fl):
                    rec["reason"] = NONFINITE
                    c["nonfinite"] += 1
                    continue
                rec["knife_q"] = min([abs(float(q) - e) for e in range(n_levels - 1)] + [np.inf])
                k.append(rec["knife_q"])
                level = 0 if fl < 0 else (n_levels - 1 if fl >= n_levels else int(fl))
                c["clamp_0" if fl < 0 else ("clamp_top" if fl >= n_levels else "level_mid")] += 1
                rec.update(in_view=1, proj_x=u, proj_y=v, proj_xr=ur, level=level, view_cos=view_cos)
                k.append(abs(float(view_cos) - 0.998))
                r0 = f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)
                c["r_25" if f64(view_cos) > 0.998 else "r_40"] += 1
                if f64(th) != 1.0:
                    r0 = r0 * th
                c["th_factor" if f64(th) != 1.0 else "th_one"] += 1
                r = r0 * sf[level]
                lvl_min, lvl_max = level - 1, level + (1 if mutant == "level_window_wide" else 0)
            else:
                oc = int(src["octave"][i])
                r0 = th
                r = th * sf[oc]
                if forward:
                    lvl_min, lvl_max = oc, 1 << 20
                    c["forward_octave_0" if oc == 0 else "forward"] += 1
                elif backward:
                    lvl_min, lvl_max = 0, oc
                    c["backward"] += 1
                else:
                    lvl_min, lvl_max = oc - 1, oc + 1
                    c["neither"] += 1
            a_x, b_x, a_y, b_y = ((u - min_x) - r) * w_inv, ((u - min_x) + r) * w_inv, ((v - min_y) - r) * h_inv, ((v - min_y) + r) * h_inv
            if np.isnan([a_x, b_x, a_y, b_y]).any():
                rec["reason"] = NONFINITE
                c["nonfinite"] += 1
                continue
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
            area = []
            for ix in range(min_cx, max_cx + 1):                   # Frame::GetFeaturesInArea, Frame.cc:387-414
                for iy in range(min_cy, max_cy + 1):
                    for j in tgt["grid"][ix][iy]:
                        if octave[j] < lvl_min or octave[j] > lvl_max:
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
            er = np.abs(ur - kr[area])
            stereo = kr[area] > 0
            if stereo.any():
                k.append(float(np.min(np.abs(er[stereo] - r) / r)))
            rec.update(area=area, octs=octave[area], hd=so.popcount_rows(tgt["desc"][area], desc_all[i]),
                       er_skip=stereo & (er > (r0 if mutant == "er_no_scale" else r)), stereo=stereo)
    return recs


def _pick(rec, blocked, opt, mutant, c):
    """the inner loop and the keep rule for one source: (choice, dist, dist2, level_best, level2, reason, knife of the ratio test)"""
    if rec["reason"] != MATCHED:
        return -1, -1, -1, -1, -1, rec["reason"], np.inf
    local = opt["mode"] == LOCAL
    best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1
    for n, idx in enumerate(rec["area"]):
        why = blocked(int(idx))
        if why:
            c[why] += 1
            continue
        if rec["er_skip"][n]:
            c["er_skip"] += 1
            continue
        c["er_pass" if rec["stereo"][n] else "kp_mono"] += 1
        d = int(rec["hd"][n])
        if (d <= best_dist and d < 256) if mutant == "best_le" else d < best_dist:
            if best_idx >= 0 and local:
                c["second_demoted"] += 1
            best_dist2, best_dist, best_level2, best_level, best_idx = best_dist, d, best_level, int(rec["octs"][n]), int(idx)
            c["best_update"] += 1
        elif local and d < best_dist2:
            best_level2, best_dist2 = int(rec["octs"][n]), d
            c["second_update"] += 1
        else:
            c["no_update"] += 1
    if best_idx < 0:
        c["none_eligible"] += 1
        return -1, -1, -1, -1, -1, NONE_ELIGIBLE, np.inf
    d2, l1, l2 = (best_dist2 if best_dist2 < 256 else -1, best_level, best_level2) if local else (-1, -1, -1)
    if best_dist > TH_HIGH:
        c["above_th"] += 1
        return -1, best_dist, d2, l1, l2, ABOVE_TH, np.inf
    knife = np.inf
    if local:
        same = best_level == best_level2 or mutant == "ratio_no_level"
        if same:
            lim = f32(opt["nn_ratio"]) * f32(best_dist2)
            knife = abs(float(best_dist) - float(lim)) / max(float(best_dist), 1.0)
            if f32(best_dist) > lim:
                c["ratio_refused"] += 1
                return -1, best_dist, d2, l1, l2, RATIO, knife
        else:
            c["ratio_level_differs"] += 1
    c["kept"] += 1
    return best_idx, best_dist, d2, l1, l2, MATCHED, knife


def _action(frame, src, opt, choice, mutant, c):
    """the writes of the loop in source order and the tail :1447-1467: (slot_src, n_matches, bin, hist, ind)"""
    ns, n = len(choice), int(np.size(frame["octave"]))
    ori = opt["mode"] == LAST and opt["check_orientation"]
    slot_src, n_matches = np.full(n, -1, np.int64), 0
    bins, hist, ind = np.full(ns, -1, np.int64), np.zeros(HISTO_LENGTH, np.int64), [-1, -1, -1]
    for i in range(ns):
        s = int(choice[i])
        if s < 0:
            continue
        if slot_src[s] >= 0:
            c["overwrite"] += 1
        if not (mutant == "first_writer" and slot_src[s] >= 0):
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
        c["maxima_3" if ind[2] >= 0 else "maxima_cut"] += 1
        for i in range(ns):
            if bins[i] >= 0 and bins[i] not in ind:
                s = int(choice[i])
                if slot_src[s] != i and slot_src[s] != -2:
                    c["nulled_overwritten"] += 1
                    if mutant == "null_skip_overwritten":
                        n_matches -= 1
                        continue
                slot_src[s] = -2
                n_matches -= 1
                c["nulled"] += 1
    return slot_src, n_matches, bins, hist, np.array(ind, np.int64)


def _result(recs, picks, action, opt, counters, extra):
    out = dict(choice=np.array([p[0] for p in picks], np.int64), dist=np.array([p[1] for p in picks], np.int64),
               dist2=np.array([p[2] for p in picks], np.int64), level_best=np.array([p[3] for p in picks], np.int64),
               level2=np.array([p[4] for p in picks], np.int64), reason=np.array([p[5] for p in picks], np.int64),
               in_view=np.array([r["in_view"] for r in recs], np.uint8), proj_x=np.array([r["proj_x"] for r in recs], f32),
               proj_y=np.array([r["proj_y"] for r in recs], f32), proj_xr=np.array([r["proj_xr"] for r in recs], f32),
               level=np.array([r["level"] for r in recs], np.int64), view_cos=np.array([r["view_cos"] for r in recs], f32),
               knife_q=np.array([r["knife_q"] for r in recs], f64),
               knife=np.array([min(r["knife"] + [p[6]]) if r["knife"] else np.inf for r, p in zip(recs, picks)], f64), counters=counters)
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
    holder_blocks = [("blocked_initial" if b else "") for b in np.asarray(frame["slot_blocked"]).reshape(-1)[:n]]
    picks = []
    for i, rec in enumerate(recs):
        p = _pick(rec, lambda idx: holder_blocks[idx], opt, mutant, c)
        picks.append(p)
        if p[0] >= 0:                                              # mvpMapPoints[bestIdx] = pMP: the slot now holds THIS point
            blocks = bool(src["blocks"][i])
            if mutant == "ignore_src_blocks":
                blocks = False
            elif mutant == "all_block":
                blocks = True
            holder_blocks[p[0]] = "blocked_by_source" if blocks else ""
    choice = [p[0] for p in picks]
    return _result(recs, picks, _action(frame, src, opt, choice, mutant, c), opt, c, {})


def rounds(frame, src, opt):
    """the parallel iteration of csrc/search_projection.hpp in numpy; n_rounds as the library counts them"""
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
            if choice[i] >= 0 and src["blocks"][i]:
                claim[choice[i]] = min(claim[choice[i]], i)
        if choice == prev:
            break
        prev = choice
    cc = _counters(opt["mode"])
    return _result(recs, picks, _action(frame, src, opt, choice, None, cc), opt, c, dict(n_rounds=n_rounds))


def differs(a, b, mode, ori=True):
    """per source: any output differs"""
    keys = [k for k in PER_SOURCE if (mode == LOCAL and k != "bin") or (mode == LAST and k in ("choice", "dist", "reason") + (("bin",) if ori else ()))]
    d = np.zeros(len(a["choice"]), bool)
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        d |= (x.view(np.uint32) != y.view(np.uint32)) if x.dtype == np.float32 else (x.astype(np.int64) != y.astype(np.int64))
    return d


def same_call(a, b, mode, ori=True):
    """every output of the call equal (floats by bits)"""
    ok = not differs(a, b, mode, ori).any() and np.array_equal(np.asarray(a["slot_src"], np.int64), np.asarray(b["slot_src"], np.int64))
    ok = ok and int(a["n_matches"]) == int(b["n_matches"])
    if mode == LAST:
        ok = ok and np.array_equal(np.asarray(a["hist"], np.int64), np.asarray(b["hist"], np.int64)) and list(a["ind"]) == list(b["ind"])
    return bool(ok)


# ---- the hand-made scene: every value chosen so that float32 arithmetic is exact ---------------------------------------------------
# Rcw is the identity with -0.0 in the third row's zeros and tcw = (0, 0, -0.0): z is exactly the point's third coordinate, sign of
# zero included.  fx = fy = 512, z = 4: u = 128 * X + 320 exactly, ur = u - 16 (mbf = 64).  5 levels at 1.5 (scale factors exact in
# float32).  LOCAL with th = 1 and a normal along the ray: radius 2.5 * 1.5^level (level 1: 3.75); LAST with th = 7: 7 * 1.5^octave
# (octave 1: 10.5).  Every case sits in a box of its own, 100 x 40 pixels; box centres lie on cell borders in x and in y.
E_K = (512.0, 512.0, 320.0, 240.0, 64.0)
E_LEVELS, E_SCALE, E_Z = 5, 1.5, 4.0
E_SF = np.array([f32(E_SCALE) ** i for i in range(E_LEVELS)], f32)
E_TH = {LOCAL: 1.0, LAST: 7.0}
OPT = {LOCAL: dict(mode=LOCAL, th=1.0, nn_ratio=0.8, view_cos_limit=0.5, check_orientation=False, mono=False, last_Rcw=np.eye(3, dtype=f32),
                   last_tcw=np.zeros(3, f32)),
       LAST: dict(mode=LAST, th=7.0, nn_ratio=0.8, view_cos_limit=0.5, check_orientation=True, mono=False, last_Rcw=np.eye(3, dtype=f32),
                  last_tcw=np.zeros(3, f32))}


def _next(x, up=True):
    return np.nextafter(f32(x), f32(np.inf if up else -np.inf))


class Builder:
    """collects key points and sources of one exact scene of one mode"""

    def __init__(self, mode, seed):
        self.mode, self.rng = mode, np.random.default_rng(seed)
        self.kps, self.srcs, self.cases, self.exact = [], [], {}, set()
        self.boxes = iter([(55.0 + 100.0 * (k % 6), 45.0 + 40.0 * (k // 6)) for k in range(66) if not (k % 6 in (2, 3) and k // 6 in (4, 5))])
        self.radius = lambda level: f32((2.5 if mode == LOCAL else 7.0) * float(E_SF[level]))

    def box(self):
        return next(self.boxes)

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def kp(self, uv, octave, desc, u_right=-1.0, blocked=False, angle=0.0):
        self.kps.append((np.array(uv, f32), int(octave), desc, f32(u_right), bool(blocked), f32(angle)))
        return len(self.kps) - 1

    def src(self, uv, desc, level=1, blocks=True, valid=True, z=E_Z, q_off=-0.5, angle=0.0, normal=None, X=None):
        """a source projecting exactly to uv (multiples of 1/64) with predicted level (LOCAL) or octave (LAST) `level`"""
        if X is None:
            X = np.array([(uv[0] - 320.0) / 128.0 * (z / E_Z), (uv[1] - 240.0) / 128.0 * (z / E_Z), z], f32)
        X = np.asarray(X, f32)
        with np.errstate(all="ignore"):
            d3 = f32(np.sqrt((f64(X[0]) * f64(X[0]) + f64(X[1]) * f64(X[1])) + f64(X[2]) * f64(X[2])))
            dmax = f32(float(d3) * E_SCALE ** (level + q_off))
            nrm = (X.astype(f64) / float(d3)).astype(f32) if normal is None else np.asarray(normal, f32)
        self.srcs.append(dict(valid=valid, blocks=blocks, Xw=X, desc=desc, normal=nrm, dist_max=dmax, dist_max_inv=f32(1.2) * dmax,
                              dist_min_inv=f32(0.8) * f32(dmax / E_SF[-1]), octave=level, angle=f32(angle)))
        return len(self.srcs) - 1

    def flip(self, d, nbits):
        return _flip(self.rng, d, nbits)

    def finish(self, name):
        kps, srcs = self.kps, self.srcs
        n = len(kps)
        frame = dict(name=name, bounds=(0.0, 640.0, 0.0, 480.0), grid=(64, 48, f32(64) / f32(640), f32(48) / f32(480)),
                     log_scale=f32(np.log(f32(E_SCALE))), scale_factors=E_SF.copy(),
                     Rcw=np.array([[1, 0, 0], [0, 1, 0], [-0.0, -0.0, 1]], f32), tcw=np.array([0, 0, -0.0], f32), Ow=np.zeros(3, f32),
                     K=np.array(E_K, f32), mb=f32(0.125),
                     kp=np.array([k[0] for k in kps], f32).reshape(-1, 2), octave=np.array([k[1] for k in kps], np.int32),
                     desc=np.array([k[2] for k in kps], np.uint8).reshape(-1, 32), u_right=np.array([k[3] for k in kps], f32),
                     slot_blocked=np.array([k[4] for k in kps], np.uint8), kp_angle=np.array([k[5] for k in kps], f32))
        src = {key: np.array([s[key] for s in srcs]) for key in ("valid", "blocks", "Xw", "desc", "normal", "dist_max", "dist_max_inv",
                                                                   "dist_min_inv", "octave", "angle")}
        src["valid"], src["blocks"] = src["valid"].astype(np.uint8), src["blocks"].astype(np.uint8)
        src["octave"] = src["octave"].astype(np.int32)
        return dict(name=name, frame=frame, src=src, opt=dict(OPT[self.mode]), cases=self.cases, exact=set(self.exact))


def _spread(b, c, level, hs, first=0, octaves=None, **kw):
    """key points along x at c + (m + 1/2) s, m = first .., s = 0.8 radius (rounded to 1/64), at Hamming distances hs from the
    descriptor D; a source at c + k s sees the key points k - 1 and k only.  Returns (D, s, key-point indices)"""
    D = b.desc()
    s = np.floor(0.8 * float(b.radius(level)) * 64) / 64
    ids = [b.kp((c[0] - 40.0 + (m + 0.5) * s, c[1]), level if octaves is None else octaves[n], b.flip(D, h), **kw) for n, (m, h) in enumerate(zip(range(first, first + len(hs)), hs))]
    return D, s, ids


def _at(c, s, k):
    return (c[0] - 40.0 + k * s, c[1])


@functools.lru_cache(maxsize=None)
def contention_scene(mode, only=None):
    """the contention cases of one mode (`only`: one group alone); cases[name] = dict(src=[...], kp=[...], want=...)"""
    b = Builder(mode, 6100 + mode)
    L = 1
    want = lambda name: only is None or only == name
    if want("pair"):                     # two sources want one key point: the later takes its second choice
        c = b.box()
        D, s, k = _spread(b, c, L, (4, 8), first=0)
        srcs = [b.src(_at(c, s, 1), D, L), b.src(_at(c, s, 1), D, L)]
        b.cases["pair"] = dict(src=srcs, kp=k, choice=[k[0], k[1]])
    if want("chain"):                    # source k prefers key point k - 1 and falls back to k: 6 rounds
        c = b.box()
        D, s, k = _spread(b, c, L, (4, 8, 16, 32, 64), first=0)
        srcs = [b.src(_at(c, s, 0.5), D, L)] + [b.src(_at(c, s, m), D, L) for m in range(1, 5)]
        b.cases["chain"] = dict(src=srcs, kp=k, choice=list(k), n_rounds=6)
    if want("fallback_above"):           # the displaced source's fallback is at 101
        c = b.box()
        D, s, k = _spread(b, c, L, (4, 101), first=0)
        srcs = [b.src(_at(c, s, 1), D, L), b.src(_at(c, s, 1), D, L)]
        b.cases["fallback_above"] = dict(src=srcs, kp=k, choice=[k[0], -1], reason=[MATCHED, ABOVE_TH], dist=[4, 101])
    if mode == LOCAL and want("fallback_ratio"):      # the displaced source's fallback fails the ratio test (40 > 0.8 * 45)
        c = b.box()
        D, s, k = _spread(b, c, L, (4, 40), first=0)
        k.append(b.kp((c[0] - 40.0 + 1.5 * s, c[1] + 1.0), L, b.flip(D, 45)))
        srcs = [b.src(_at(c, s, 1), D, L), b.src(_at(c, s, 1), D, L)]
        b.cases["fallback_ratio"] = dict(src=srcs, kp=k, choice=[k[0], -1], reason=[MATCHED, RATIO], dist=[4, 40])
    if mode == LOCAL and want("second_blocked"):      # the SECOND best is taken by an earlier source: the ratio test flips to keep
        c = b.box()
        D, s, k = _spread(b, c, L, (40, 45), first=0)
        srcs = [b.src(_at(c, s, 2), D, L), b.src(_at(c, s, 1), D, L), b.src(_at(c, s, 1), D, L, valid=False)]
        b.cases["second_blocked"] = dict(src=srcs, kp=k, choice=[k[1], k[0], -1], reason=[MATCHED, MATCHED, INVALID_SRC])
    if want("overwritten"):              # a non-blocking source (a temporal point) is over-written by a later one: both counted
        c = b.box()
        D, s, k = _spread(b, c, L, (4,), first=0)
        srcs = [b.src(_at(c, s, 0.5), D, L, blocks=False), b.src(_at(c, s, 0.5), D, L)]
        b.cases["overwritten"] = dict(src=srcs, kp=k, choice=[k[0], k[0]], slot_src={k[0]: srcs[1]})
    if want("blocked_initially"):        # the best slot held an observed point before the call
        c = b.box()
        D, s, k = _spread(b, c, L, (4,), first=0, blocked=True)
        k.append(b.kp((c[0] - 40.0 + 0.5 * s, c[1] + 1.0), L - 1, b.flip(D, 9)))
        srcs = [b.src(_at(c, s, 0.5), D, L)]
        b.cases["blocked_initially"] = dict(src=srcs, kp=k, choice=[k[1]])
    if want("zero_obs_slot"):            # the slot held a 0-observation point (slot_blocked 0): taken like an empty one
        c = b.box()
        D, s, k = _spread(b, c, L, (6,), first=0)
        srcs = [b.src(_at(c, s, 0.5), D, L)]
        b.cases["zero_obs_slot"] = dict(src=srcs, kp=k, choice=[k[0]])
    if mode == LAST and want("ori"):     # 12 plain matches in bin 0, 3 in bin 6, and an over-written slot whose first writer is alone in bin 3
        for m in range(15):
            c = b.box()
            D, s, k = _spread(b, c, L, (3 + m % 5,), first=0)
            b.src(_at(c, s, 0.5), D, L, angle=(200.0 if m >= 12 else 10.0 + m), blocks=bool(m % 2))
            b.kps[k[0]] = b.kps[k[0]][:5] + (f32(20.0 if m >= 12 else 10.0 + m + (5.0 if m % 3 == 0 else -5.0)),)
        c = b.box()
        D, s, k = _spread(b, c, L, (4,), first=0)
        srcs = [b.src(_at(c, s, 0.5), D, L, blocks=False, angle=90.0), b.src(_at(c, s, 0.5), D, L, angle=1.0)]
        b.cases["ori_overwritten"] = dict(src=srcs, kp=k, choice=[k[0], k[0]], slot_src={k[0]: -2}, bin=[3, 0])
        for name, a_src, a_kp, want_bin in (("bin_wrap", 900.0, 0.0, 0), ("bin_31", 930.0, 0.0, -1), ("bin_nan", np.nan, 0.0, -1), ("rot_neg", 5.0, 355.0, 0)):
            c = b.box()
            D, s, k = _spread(b, c, L, (5,), first=0)
            b.kps[k[0]] = b.kps[k[0]][:5] + (f32(a_kp),)
            srcs = [b.src(_at(c, s, 0.5), D, L, angle=a_src)]
            b.cases[name] = dict(src=srcs, kp=k, choice=[k[0]], bin=[want_bin], slot_src={k[0]: srcs[0]})
    return b.finish("contention" if only is None else only)


@functools.lru_cache(maxsize=None)
def edge_scene(mode):
    """ties, stereo and mono key points, levels 0 and top, the octave windows, the exact thresholds, the refusals and the cases
    where the reference is undefined"""
    b = Builder(mode, 6200 + mode)
    L = 1
    R = float(b.radius(L))
    # ties across cell x, cell y and index: the LOWER index lies later in the traversal (octaves differ: LOCAL's ratio test passes)
    for name, off_a, off_b, first in (("tie_cx", (1.0, 1.5), (-1.0, 1.5), 1), ("tie_cy", (1.5, 1.0), (1.0, -1.0), 1), ("tie_cell", (1.0, 1.0), (2.0, 2.0), 0)):
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + off_a[0], c[1] + off_a[1]), L, b.flip(D, 7)), b.kp((c[0] + off_b[0], c[1] + off_b[1]), L - 1, b.flip(D, 7))]
        b.cases[name] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[first]], dist=[7])
    # the same tie at one level: LOCAL refuses it by the ratio test (7 > 0.8 * 7)
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 1.0, c[1] + 1.0), L, b.flip(D, 7)), b.kp((c[0] + 2.0, c[1] + 2.0), L, b.flip(D, 7))]
    b.cases["tie_same_level"] = dict(src=[b.src(c, D, L)], kp=k, choice=[-1 if mode == LOCAL else k[0]])
    # the 100 limit
    for name, h in (("th_100", 100), ("th_101", 101)):
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] - 0.25), L, b.flip(D, h))]
        b.cases[name] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[0] if h == 100 else -1], dist=[h], reason=[MATCHED if h == 100 else ABOVE_TH])
    # the ratio at equality: 0.8f * 50 rounds to 40.0f, and 40 > 40 is false
    if mode == LOCAL:
        for name, h in (("ratio_eq", 40), ("ratio_above", 41)):
            c = b.box()
            D = b.desc()
            k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, h)), b.kp((c[0] - 0.5, c[1] - 0.5), L, b.flip(D, 50))]
            si = b.src(c, D, L)
            b.cases[name] = dict(src=[si], kp=k, choice=[k[0] if h == 40 else -1], reason=[MATCHED if h == 40 else RATIO])
            b.exact.add(si)
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
    # er == radius exactly passes (`er > radius` skips); one step more is skipped; u_right == 0 and < 0 are monocular; a far u_right
    for name, hit in (("er_eq_r", True), ("er_above_r", False)):
        c = b.box()
        D = b.desc()
        ur = f32(f32(c[0]) - f32(16.0))
        kr = f32(ur + f32(R)) if hit else _next(ur + f32(R))
        assert (abs(ur - kr) > f32(R)) != hit and kr > 0
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 5), u_right=kr)]
        si = b.src(c, D, L)
        b.cases[name] = dict(src=[si], kp=k, choice=[k[0] if hit else -1], reason=[MATCHED if hit else NONE_ELIGIBLE])
        b.exact.add(si)
    c = b.box()
    D = b.desc()
    k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 3), u_right=c[0] + 60.0), b.kp((c[0] - 0.5, c[1] + 0.5), L - 1, b.flip(D, 9), u_right=0.0),
         b.kp((c[0] - 1.0, c[1] - 0.5), L - 1, b.flip(D, 20), u_right=-1.0), b.kp((c[0] + 1.0, c[1] - 0.5), L - 1, b.flip(D, 30), u_right=c[0] - 15.0)]
    b.cases["stereo_mixed"] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[1]], dist=[9])
    # u == max_x exactly is inside (closed), one float32 above is outside; v likewise; u == min_x is inside
    for name, X0, inside in (("u_eq_max", 2.5, True), ("u_above_max", 2.5 + 2.0 ** -21, False)):
        si = b.src((640.0, 200.0), b.desc(), L, X=(X0, (200.0 - 240.0) / 128.0, E_Z))
        b.cases[name] = dict(src=[si], reason=[EMPTY if inside else OUTSIDE])
        b.exact.add(si)
    for name, Y0, inside in (("v_eq_max", 1.875, True), ("v_above_max", 1.875 + 2.0 ** -21, False)):
        si = b.src((100.0, 480.0), b.desc(), L, X=((100.0 - 320.0) / 128.0, Y0, E_Z))
        b.cases[name] = dict(src=[si], reason=[EMPTY if inside else OUTSIDE])
        b.exact.add(si)
    si = b.src((0.0, 300.0), b.desc(), L)
    b.cases["u_eq_min"] = dict(src=[si], reason=[EMPTY])
    b.exact.add(si)
    # z == +0.0 / -0.0: LOCAL lets both pass `PcZ < 0` (u is infinite: outside); LAST refuses -0.0 (invzc = -inf < 0).  With x == 0 too,
    # u = 0 * inf is NaN, which passes every compare of the reference
    for name, X, why in (("z_plus_0", (0.5, 0.5, 0.0), {LOCAL: OUTSIDE, LAST: OUTSIDE}), ("z_minus_0", (0.5, 0.5, -0.0), {LOCAL: OUTSIDE, LAST: Z_NEG}),
                         ("z_0_x_0", (0.0, 0.0, 0.0), {LOCAL: NONFINITE, LAST: NONFINITE}), ("x_nan", (np.nan, 0.0, 4.0), {LOCAL: NONFINITE, LAST: NONFINITE}),
                         ("z_tiny_neg", (0.5, 0.5, -float(np.finfo(f32).tiny)), {LOCAL: Z_NEG, LAST: Z_NEG})):
        si = b.src(None, b.desc(), L, X=X, normal=(0.0, 0.0, 1.0))
        b.cases[name] = dict(src=[si], reason=[why[mode]])
        b.exact.add(si)
    si = b.src(b.box(), b.desc(), L, valid=False)
    b.cases["invalid"] = dict(src=[si], reason=[INVALID_SRC])
    si = b.src(None, b.desc(), L, X=((-300.0 - 320.0) / 128.0, 0.0, E_Z))
    b.cases["u_below_min"] = dict(src=[si], reason=[OUTSIDE])
    si = b.src(None, b.desc(), L, X=(0.0, (-5.0 - 240.0) / 128.0, E_Z))
    b.cases["v_below_min"] = dict(src=[si], reason=[OUTSIDE])
    si = b.src(b.box(), b.desc(), L)
    b.cases["empty_box"] = dict(src=[si], reason=[EMPTY])
    si = b.src(None, b.desc(), 4, X=((639.0 - 320.0) / 128.0, (479.0 - 240.0) / 128.0, E_Z))
    b.cases["corner"] = dict(src=[si], reason=[EMPTY])
    # a key point never filed (round(636 / 10) == 64 == grid_cols) with the perfect descriptor next to a filed one
    D = b.desc()
    si = b.src(None, D, L, X=((633.0 - 320.0) / 128.0, (100.0 - 240.0) / 128.0, E_Z))
    k = [b.kp((636.0, 100.0), L, D.copy()), b.kp((632.0, 100.5), L, b.flip(D, 30))]
    b.cases["unfiled"] = dict(src=[si], kp=k, choice=[k[1]], dist=[30])
    if mode == LOCAL:
        # the distance limits: equal passes, one step inside refuses
        for name, which, step, ok in (("d_eq_min", "dist_min_inv", 0, True), ("d_eq_max", "dist_max_inv", 0, True),
                                      ("d_below_min", "dist_min_inv", 1, False), ("d_above_max", "dist_max_inv", -1, False)):
            c = b.box()
            D = b.desc()
            si = b.src(c, D, L)
            X = b.srcs[si]["Xw"]
            d3 = f32(np.sqrt((f64(X[0]) * f64(X[0]) + f64(X[1]) * f64(X[1])) + f64(X[2]) * f64(X[2])))
            b.srcs[si][which] = d3 if step == 0 else _next(d3, step > 0)
            k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 3))]
            b.cases[name] = dict(src=[si], kp=k, choice=[k[0] if ok else -1], reason=[MATCHED if ok else DISTANCE])
            b.exact.add(si)
        # viewCos: on the axis PO = (0, 0, 4) and the normal (., 0, c) give viewCos = c exactly.  One float32 step either side of the
        # limit 0.5 and of 0.998 (float32(0.998) is above the double 0.998: radius 2.5; the step below: radius 4).  A key point 3.9
        # pixels off lies inside 4 * 1.5 and outside 2.5 * 1.5.  The sources do not block, so all of them see it.
        D = b.desc()
        k = [b.kp((323.90625, 240.0), L, b.flip(D, 2))]
        for name, cz, why, hit in (("cos_eq_limit", f32(0.5), MATCHED, True), ("cos_below_limit", _next(0.5, False), ANGLE, False),
                                   ("cos_above_998", f32(0.998), EMPTY, False), ("cos_below_998", _next(f32(0.998), False), MATCHED, True)):
            assert (f64(cz) > 0.998) == (name == "cos_above_998")
            si = b.src((320.0, 240.0), D, L, blocks=False, normal=(np.sqrt(1.0 - float(cz) ** 2), 0.0, cz))
            b.cases[name] = dict(src=[si], kp=k, choice=[k[0] if hit else -1], reason=[why], view_cos=cz)
            b.exact.add(si)
        si = b.src((320.0, 240.0), D, L, blocks=False)
        b.srcs[si]["dist_max"] = f32(np.nan)
        b.cases["dist_max_nan"] = dict(src=[si], reason=[NONFINITE])
        b.exact.add(si)
        # the level clamped at 0 and at the top: the window is the CLAMPED level's; perfect descriptors wait one level outside it
        for name, q, lvl in (("clamp_0", -2.6, 0), ("clamp_top", 7.3, E_LEVELS - 1)):
            c = b.box()
            D = b.desc()
            si = b.src(c, D, 0, q_off=q)
            b.srcs[si]["dist_min_inv"], b.srcs[si]["dist_max_inv"] = f32(0.01), f32(1000.0)
            k = [b.kp((c[0] + 0.5, c[1] - 0.5), lvl, b.flip(D, 9)), b.kp((c[0] - 0.5, c[1] + 0.5), 1 if lvl == 0 else lvl - 2, D.copy())]
            b.cases[name] = dict(src=[si], kp=k, choice=[k[0]], dist=[9], level=lvl)
        # level + 1 holds the perfect descriptor: outside the window level - 1 .. level
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), 2, b.flip(D, 11)), b.kp((c[0] - 0.5, c[1] - 0.5), 3, D.copy()), b.kp((c[0] - 0.5, c[1] + 0.5), 0, D.copy())]
        b.cases["window"] = dict(src=[b.src(c, D, 2)], kp=k, choice=[k[0]], dist=[11])
        # best and second at one level pass the ratio test (8 <= 0.8 * 20); at different levels it is not applied (19 against 20)
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 20)), b.kp((c[0] - 0.5, c[1] - 0.5), L, b.flip(D, 8)), b.kp((c[0] - 0.5, c[1] + 0.5), L, b.flip(D, 30))]
        b.cases["ratio_pass"] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[1]], dist=[8], dist2=[20])
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + 0.5, c[1] + 0.5), L, b.flip(D, 20)), b.kp((c[0] - 0.5, c[1] - 0.5), L - 1, b.flip(D, 19))]
        b.cases["ratio_levels_differ"] = dict(src=[b.src(c, D, L)], kp=k, choice=[k[1]], dist=[19], dist2=[20])
    else:
        # octaves o - 2 .. o + 2 around a source of octave 2: forward takes o + 2 (distance 1), backward o - 2 (2), neither o + 1 (8)
        c = b.box()
        D = b.desc()
        k = [b.kp((c[0] + dx, c[1] + dy), o, b.flip(D, h)) for (dx, dy), o, h in zip(((1, 1), (-1, 1), (1, -1), (-1, -1), (0.5, 0)), (0, 1, 2, 3, 4), (2, 12, 20, 8, 1))]
        b.cases["windows"] = dict(src=[b.src(c, D, 2)], kp=k, by_direction=dict(forward=k[4], backward=k[0], neither=k[3]))
        # octave 0 (forward: unchecked) and the top octave
        for name, o in (("octave_0", 0), ("octave_top", E_LEVELS - 1)):
            c = b.box()
            D = b.desc()
            k = [b.kp((c[0] + 0.5, c[1] + 0.5), o, b.flip(D, 10)), b.kp((c[0] - 0.5, c[1] - 0.5), 2, b.flip(D, 5))]
            b.cases[name] = dict(src=[b.src(c, D, o)], kp=k)
    return b.finish("edges")


DIRECTIONS = dict(neither=dict(last_tcw=(0.0, 0.0, 0.0)), forward=dict(last_tcw=(0.0, 0.0, 0.5)), backward=dict(last_tcw=(0.0, 0.0, -0.5)),
                  mono=dict(last_tcw=(0.0, 0.0, 0.5), mono=True))


# ---- the random scenes: the frames and the pool of tests/fuse_oracle.py (a rotated pose, three pyramids and grids) ---------------------
def random_scene(mode, spec_index=0, n=None, seed=0, th=None):
    """frame: fo.make_target (own pose near the base camera, mono and stereo key points mixed) with a fifth of the slots taken at
    entry; sources: fo.main_pool() in order, a tenth invalid, a third not blocking"""
    spec = fo.SPEC[spec_index] if seed == 0 else dict(fo.SPEC[spec_index], seed=seed)
    T, pool = fo.make_target(spec, n=n), fo.main_pool()
    rng = np.random.default_rng(70000 + 10 * spec_index + mode + 100 * seed)
    nk, ns = len(T["octave"]), fo.N_POOL
    frame = dict(T, slot_blocked=(rng.random(nk) < 0.2).astype(np.uint8), kp_angle=rng.uniform(0, 360, nk).astype(f32), mb=f32(0.08))
    frame["u_right"] = np.where(np.arange(nk) % 7 == 3, f32(0.0), T["u_right"]).astype(f32)
    levels = len(T["scale_factors"])
    src = dict(valid=(rng.random(ns) < 0.9).astype(np.uint8), blocks=(rng.random(ns) < 0.67).astype(np.uint8), Xw=pool["Xw"], desc=pool["desc"],
               normal=pool["normal"], dist_min_inv=pool["dist_min_inv"], dist_max_inv=pool["dist_max_inv"], dist_max=pool["dist_max"],
               octave=np.minimum(pool["level"], levels - 1).astype(np.int32), angle=rng.uniform(0, 360, ns).astype(f32))
    opt = dict(OPT[mode], th=(3.0 if mode == LOCAL else 15.0) if th is None else th)
    if mode == LAST:
        R, t = np.asarray(T["Rcw"], f32), np.asarray(T["tcw"], f32)
        opt.update(last_Rcw=R, last_tcw=(t + np.array((0.0, 0.0, (0.3, -0.3, 0.01)[spec_index]), f32)).astype(f32))
    return dict(name="random %d" % spec_index, frame=frame, src=src, opt=opt, cases={}, exact=set())


STRIDE_N = (0, 1, 63, 64, 65, 4097)


@functools.lru_cache(maxsize=None)
def fixtures(mode):
    """name -> dict(frame, src, opt, cases, exact); treat as read-only"""
    out = dict(contention=contention_scene(mode), chain=contention_scene(mode, "chain"), edges=edge_scene(mode))
    variant = lambda f, name, **o: dict(f, name=name, opt=dict(f["opt"], **o), cases={} if o else f["cases"])
    if mode == LOCAL:
        out["edges_th3"] = variant(out["edges"], "edges_th3", th=3.0)
    else:
        for d, o in DIRECTIONS.items():
            out["edges_" + d] = variant(out["edges"], "edges_" + d, **(o if d != "neither" else {}))
        del out["edges"]
        out["contention_no_ori"] = variant(out["contention"], "contention_no_ori", check_orientation=False)
    # a grid that covers only the left half of the image (cells of 5 pixels): sources beyond it have no cell range at all
    e = out["edges" if mode == LOCAL else "edges_neither"]
    out["edges_half_grid"] = dict(e, name="edges_half_grid", cases={}, frame=dict(e["frame"], grid=(64, 48, f32(0.2), f32(0.2))))
    for s in range(3):
        out["random_%d" % s] = random_scene(mode, s, seed=(0, 0, 5)[s])   # (a pose of the third frame whose level decisions keep THRESHOLD)
    out["random_th1"] = random_scene(mode, 0, th=1.0 if mode == LOCAL else 7.0)
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


def take_sources(src, idx):
    return {k: np.asarray(v)[idx] for k, v in src.items()}


def weave(f, mode):
    """the fixture with unrelated gated-out sources woven in (an invalid one, one behind the camera, one outside the image, in turn,
    before every source).  Returns (fixture, positions of the original sources)"""
    src, ns = f["src"], int(np.size(f["src"]["valid"]))
    extra = take_sources(src, np.arange(ns) % max(ns, 1))
    extra = {k: v.copy() for k, v in extra.items()}
    R, t = np.asarray(f["frame"]["Rcw"], f64).reshape(3, 3), np.asarray(f["frame"]["tcw"], f64).reshape(3)
    for i in range(ns):
        if i % 3 == 0:
            extra["valid"][i] = 0
        else:
            Y = np.array((0.3, 0.2, -3.0)) if i % 3 == 1 else np.array((40.0, 0.1, 4.0))
            extra["Xw"][i] = (R.T @ (Y - t)).astype(f32)
            extra["valid"][i] = 1
    woven = {k: np.stack([extra[k], np.asarray(src[k])], 1).reshape((2 * ns,) + np.asarray(src[k]).shape[1:]) for k in src}
    return dict(f, src=woven), np.arange(ns) * 2 + 1
