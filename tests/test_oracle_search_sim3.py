"""CPU: the conditions on tests/search_sim3_oracle.py under which tests/test_gpu_search_sim3.py decides anything -- the two flavours
agree outside the band, at most 2 % of a candidate's source slots lie inside it, every edge case the kernel can go wrong at occurs
in the pool, and the brute-force form with the 64-bit key (what csrc/search_sim3.hpp computes) equals the literal grid walk."""
import json

import numpy as np

from tests import search_sim3_oracle as so


def test_flavours_agree_outside_the_band():
    width = so.band()
    print("measured band %.3e, BAND %.3e" % (so.measured(), width))
    for i, (a, b) in enumerate(zip(so.pool_results("f32"), so.pool_results("f64"))):
        for d, diff in zip((1, 2), so.disagreements(a, b)):
            assert not (diff & (b["knife%d" % d] >= width) & (width > 0)).any() and (width > 0 or not diff.any()), (i, d)
        share = so.in_band_share(b, width)
        print("candidate %2d: %.4f of the source slots inside the band" % (i, share))
        assert share <= so.IN_BAND_CAP, (i, share)


def test_brute_force_key_equals_the_grid_walk():
    for flavour in ("f32", "f64"):
        for i, (g, b) in enumerate(zip(so.pool_results(flavour), so.pool_results(flavour, "brute"))):
            for key in ("best1", "dist1", "best2", "dist2", "match12"):
                assert np.array_equal(g[key], b[key]), (flavour, i, key)
            assert g["n_found"] == b["n_found"]


def test_every_edge_case_occurs():
    pool, res = so.pool(), so.pool_results("f64")
    assert [len(c["kf2"]["octave"]) for c in pool[:7]] == [0, 1, 63, 64, 65, 129, 300] and len(so.key_frame_1()["octave"]) == 130
    reasons = np.concatenate([np.concatenate([r["reason1"], r["reason2"]]) for r in res])
    count = {name: int((reasons == k).sum()) for k, name in enumerate(so.REASONS)}
    print(count)
    assert all(count[name] >= 2 for name in so.REASONS), count
    assert not pool[7]["kf2"]["has_point"].any() and res[7]["n_found"] == 0 and (res[7]["best1"] >= 0).any()
    assert pool[8]["pre1"].all() and (res[8]["best1"] == -1).all() and (res[8]["best2"] >= 0).any() and res[8]["n_found"] == 0
    infos = [inf for r in res for d in ("info1", "info2") for inf in r[d].values()]
    assert sum(inf["q"] <= -1 and inf["level"] == 0 for inf in infos) >= 2                       # clamped at 0
    assert sum(inf["q"] > so.N_LEVELS and inf["level"] == so.N_LEVELS - 1 for inf in infos) >= 2   # clamped at the top
    assert sum(inf["unfiled_in_box"] > 0 for inf in infos) >= 2
    assert sum(inf["octaves"] == [-2, -1, 0, 1] for inf in infos) >= 1
    assert sum(inf["tie"] for inf in infos) >= 3 and sum(inf["tie_same_cx"] for inf in infos) >= 1
    small = res[so.I_SMALL]["info1"].values()                                                      # 128 x 96 on the 64 x 48 grid
    assert pool[so.I_SMALL]["kf2"]["bounds"] == (0.0, 128.0, 0.0, 96.0) and tuple(pool[so.I_SMALL]["kf2"]["grid"][:2]) == (64, 48)
    assert any(i["lo_x"] < 0 for i in small) and any(i["hi_x"] > 63 for i in small)
    assert any(i["lo_y"] < 0 for i in small) and any(i["hi_y"] > 47 for i in small)
    dists = np.concatenate([np.concatenate([r["dist1"], r["dist2"]]) for r in res])
    assert (dists == 100).any() and (dists == 101).any()
    assert sum(int(((r["best1"] >= 0) & (r["match12"] < 0)).sum()) for r in res) >= 3            # agreement that fails


def test_the_named_cases():
    sp, r = so.special_candidate(), so.pool_results("f64")[so.I_SPECIAL]
    n = so.NAMED
    for name, first in sp["tie_first"].items():                # an index-only tie-break would return tie_lowest
        assert r["best1"][n[name]] == first != sp["tie_lowest"][name] and first > sp["tie_lowest"][name], name
        assert r["info1"][n[name]]["tie"]
    assert r["info1"][n["tie_cy"]]["tie_same_cx"]
    assert r["dist1"][n["th_100"]] == 100 and r["best1"][n["th_100"]] >= 0
    assert r["dist1"][n["th_101"]] == 101 and r["best1"][n["th_101"]] == -1
    assert r["best1"][n["unfiled"]] == sp["unfiled_filed"] and r["dist1"][n["unfiled"]] == 40
    assert r["info1"][n["unfiled"]]["unfiled_in_box"] == 1
    assert r["dist1"][n["octaves"]] == 20                     # the distance-0 key points at level - 2 and level + 1 do not count
    assert r["best1"][n["no_mutual"]] >= 0 and r["best2"][r["best1"][n["no_mutual"]]] not in (-1, n["no_mutual"])
    assert r["match12"][n["no_mutual"]] == -1
    pb = sp["pre2_best"]
    assert r["best1"][n["pre2_best"]] == pb and r["best2"][pb] == -1 and r["match12"][n["pre2_best"]] == -1
    assert r["reason1"][n["empty_box"]] == so.EMPTY
    assert r["match12"][n["tie_cx"]] == sp["tie_first"]["tie_cx"] and r["n_found"] == 1


# ---- the mixed pool (so.POOL_MIXED): frames and candidates that differ from each other ------------------------------------------
# what POOL notices of each mutant of so.one_pass: nothing of the first four (its frames share one pyramid, its candidates one
# camera and one th, and no key point waits at a level below 0), the others through the clamped slots of key frame 1 and the
# 64 x 48 grid
OLD_POOL_MISSES = ("src_pyramid", "cand0_K", "cand0_th", "no_lower_clamp")
OLD_POOL_CATCHES = ("swap_rows_cols", "no_upper_clamp", "gate_unclamped")


def test_mixed_flavours_agree_outside_the_band():
    width = so.band_mixed()
    print("mixed pool: measured band %.3e, BAND %.3e" % (so.measured_mixed(), width))
    for i, (a, b) in enumerate(zip(so.pool_mixed_results("f32"), so.pool_mixed_results("f64"))):
        for d, diff in zip((1, 2), so.disagreements(a, b)):
            assert not (diff & (b["knife%d" % d] >= width) & (width > 0)).any() and (width > 0 or not diff.any()), (i, d)
        share = so.in_band_share(b, width)
        print("mixed candidate %d (%s): %.4f of the source slots inside the band" % (i, so.POOL_MIXED[i]["name"], share))
        assert share <= so.IN_BAND_CAP, (i, share)
    doc = json.load(open(so.MARGINS))["search_sim3/mixed/band_f32_vs_f64"]                   # the committed copy
    assert doc["measured"] == so.measured_mixed() and doc["tol"] == width


def test_mixed_brute_force_key_equals_the_grid_walk():
    for flavour in ("f32", "f64"):
        for i, (g, b) in enumerate(zip(so.pool_mixed_results(flavour), so.pool_mixed_results(flavour, "brute"))):
            for key in ("best1", "dist1", "best2", "dist2", "match12"):
                assert np.array_equal(g[key], b[key]), (flavour, i, key)
            assert g["n_found"] == b["n_found"]


def _caught(true, mutant, width):
    """per candidate and direction: the slots outside the band on which a mutant's result differs from the true one"""
    return [[np.nonzero(diff & (t["knife%d" % d] > width))[0] for d, diff in zip((1, 2), so.disagreements(t, m))] for t, m in zip(true, mutant)]


def test_every_mutant_is_caught_by_the_mixed_pool_and_what_the_old_pool_misses():
    assert set(OLD_POOL_MISSES) | set(OLD_POOL_CATCHES) == set(so.MUTANTS)
    true, old = so.pool_mixed_results("f64", "brute"), so.pool_results("f64", "brute")
    n = len(true)
    for m in so.MUTANTS:
        c = _caught(true, so.pool_mixed_results("f64", "brute", m), so.band_mixed())
        c_old = _caught(old, so.pool_mutant_results(m), so.band())
        n_old = sum(len(s) for cd in c_old for s in cd)
        print("%-15s mixed pool: %s   old pool: %d slots" % (m, [(len(a), len(b)) for a, b in c], n_old))
        assert sum(len(s) for cd in c for s in cd) >= 1, m
        if m in OLD_POOL_MISSES:                               # the gap: the old pool's every output is the same under this mutant
            for t, r in zip(old, so.pool_mutant_results(m)):
                assert all(np.array_equal(t[k], r[k]) for k in ("best1", "dist1", "best2", "dist2", "match12")) and t["n_found"] == r["n_found"], m
        else:
            assert n_old >= 1, m
        # ... and by every candidate and direction in which the mistake reads another value at all
        if m == "src_pyramid":
            want = [(i, d) for i in range(n) for d in (0, 1) if so.POOL_MIXED[i]["levels"] != so.N_LEVELS or so.POOL_MIXED[i]["scale"] != 1.2]
            assert len(want) == 2 * (n - 1)
        elif m == "cand0_K":
            want = [(i, d) for i in range(1, n) for d in (0, 1)]
        elif m == "cand0_th":                                  # through the key points planted between two values of th
            want = [(i, 0) for i in range(1, n) if so.POOL_MIXED[i]["th"] != so.POOL_MIXED[0]["th"]]
            for i, _ in want:
                nm = so.pool_mixed()[i]["named"]
                th0, th = so.POOL_MIXED[0]["th"], so.POOL_MIXED[i]["th"]
                assert th0 < th or (nm["th_out"] and nm["th_out"][0] in c[i][0]), i      # a larger th admits the perfect key point
                assert th0 > th or (nm["th_in"] and nm["th_in"][0] in c[i][0]), i        # a smaller one drops the only key point
            assert len({s["th"] for s in so.POOL_MIXED}) >= 3
        elif m == "swap_rows_cols":                            # the pass into key frame 1 (64 x 48) and into every grid that is not square
            want = [(i, 1) for i in range(n)] + [(i, 0) for i in range(n) if so.POOL_MIXED[i]["grid"][0] != so.POOL_MIXED[i]["grid"][1]]
        else:                                                  # the clamps: both directions somewhere, counted below
            want = []
            assert any(len(cd[0]) for cd in c) and any(len(cd[1]) for cd in c), m
        for i, d in want:
            assert len(c[i][d]) >= 1, (m, i, d)


def test_mixed_pool_clamps_and_levels():
    pool, res = so.pool_mixed(), so.pool_mixed_results("f64")
    src = so.pool_mixed_results("f64", "brute", "src_pyramid")
    top_by_levels = {}
    for i, (c, r) in enumerate(zip(pool, res)):
        for d, nl in ((1, so.POOL_MIXED[i]["levels"]), (2, so.N_LEVELS)):
            inf = r["info%d" % d]
            low = sum(v["q"] <= -1 and v["level"] == 0 for v in inf.values())
            top = sum(v["q"] >= nl and v["level"] == nl - 1 for v in inf.values())
            other = src[i]["info%d" % d]
            differ = np.mean([inf[s]["level"] != other[s]["level"] for s in inf if s in other])
            print("mixed candidate %d (%s) pass %d: %d slots clamped at level 0, %d at the top level, %.2f of the levels differ from the "
                  "source pyramid's" % (i, so.POOL_MIXED[i]["name"], d, low, top, differ))
            if d == 1:
                top_by_levels[nl] = top_by_levels.get(nl, 0) + top
            else:
                assert low >= 2 and top >= 2, (i, low, top)                  # planted: log(ratio) / log_scale = -2.5 and 9.4
            if (nl if d == 1 else so.POOL_MIXED[i]["levels"]) != so.N_LEVELS or so.POOL_MIXED[i]["scale"] != 1.2:
                assert differ >= 1 / 3, (i, d, differ)
        g = c["named"]["gates"]
        # level 0, log(ratio) / log_scale well below 0: the octave-0 key point wins over the perfect descriptor at octave 1
        if so.POOL_MIXED[i].get("s12") != 1.6:
            s = so.S_CLAMP0
            assert g[s]["q"] <= -1.2 and g[s]["level"] == 0 and r["info1"][s]["level"] == 0
            assert r["best1"][s] == g[s]["winner"] and r["dist1"][s] == 12 and (g[s]["above"] is not None or so.POOL_MIXED[i]["levels"] == 1)
        for s in so.S_GATES:                                   # wherever a gate source is searched, the perfect descriptors lose
            if r["reason1"][s] == so.SEARCHED:
                assert r["best1"][s] == g[s]["winner"] and r["dist1"][s] == 12, (i, s)
    print("pass 1 -> 2, slots clamped at the top level by n_levels:", top_by_levels)
    assert all(top_by_levels[nl] >= 1 for nl in (1, 5, 16)), top_by_levels
    for i in (0, 1, 2):                                        # 5, 16 and 1 levels: the planted source at the top
        s, g, nl = so.S_CLAMPTOP, pool[i]["named"]["gates"], so.POOL_MIXED[i]["levels"]
        assert g[s]["q"] >= nl and g[s]["level"] == nl - 1 and res[i]["best1"][s] == g[s]["winner"], i
        assert nl < 3 or g[s]["below"] is not None
    one = res[2]["info1"]                                      # one level: both clamps give level 0
    assert any(v["q"] <= -1 for v in one.values()) and any(v["q"] >= 1 for v in one.values()) and all(v["level"] == 0 for v in one.values())


def test_mixed_pool_coverage():
    pool, res, k1 = so.pool_mixed(), so.pool_mixed_results("f64"), so.key_frame_1()
    assert all(len(c["kf2"]["octave"]) == so.N2_MIXED <= 130 for c in pool)
    reasons = np.concatenate([np.concatenate([r["reason1"], r["reason2"]]) for r in res])
    count = {name: int((reasons == k).sum()) for k, name in enumerate(so.REASONS)}
    print(count)
    assert all(count[name] >= 2 for name in so.REASONS), count
    assert [(s["levels"], round(s["scale"], 3)) for s in so.POOL_MIXED[:4]] == [(5, 1.5), (16, 1.1), (1, 1.2), (8, 1.414)]
    assert {tuple(s["grid"]) for s in so.POOL_MIXED} >= {(1, 1), (5, 7), (64, 64), (64, 48)}
    assert any(s["bounds"][0] < 0 and s["bounds"][2] < 0 and s["bounds"][0] != int(s["bounds"][0]) for s in so.POOL_MIXED)
    # cameras: every pair of candidates differs by more than the largest search radius in a focal length or a centre
    for i, a in enumerate(pool):
        for j, b in enumerate(pool[:i]):
            r_max = max(float(c["th"]) * float(c["kf2"]["scale_factors"][-1]) for c in (a, b))
            assert np.abs(a["K"][2:] - b["K"][2:]).max() > 25 or np.abs(a["K"][:2] - b["K"][:2]).max() * 0.3 > r_max, (i, j)
    assert len({tuple(c["K"]) for c in pool}) == len(pool) and len({float(c["th"]) for c in pool}) >= 3
    for i, (c, r) in enumerate(zip(pool, res)):
        nm = c["named"]
        if nm["th_in"]:                                        # inside the box at this th (outside at the next smaller): found
            assert r["best1"][nm["th_in"][0]] == nm["th_in"][1] and r["dist1"][nm["th_in"][0]] == 6, i
        if nm["th_out"]:                                       # the perfect one outside the box at this th (inside at the next larger)
            assert r["best1"][nm["th_out"][0]] == nm["th_out"][1] and r["dist1"][nm["th_out"][0]] == 9, i
        assert nm["th_in"] or nm["th_out"]
        if so.POOL_MIXED[i]["span"] is None:                        # matched key points in the first and last filed row and column
            cx, cy, ok = so.cells(c["kf2"])
            b = r["best1"][r["best1"] >= 0]
            cols, rows = so.POOL_MIXED[i]["grid"]
            assert ok[b].all() and (cx[b] == 0).any() and (cx[b] == cols - 1).any() and (cy[b] == 0).any() and (cy[b] == rows - 1).any(), i
            assert (~ok).any()                                 # and key points in the half cell that is never filed
            if so.POOL_MIXED[i]["bounds"][0] < 0:
                kp = c["kf2"]["kp"][b]
                assert (kp[:, 0] < 0).any() and (kp[:, 1] < 0).any()
    # the 1 x 1 grid: of two equal distances the lower index wins; over a 64 x 48 grid the smaller cell x (the higher index) would
    c, r = pool[so.I_1X1], res[so.I_1X1]
    s, a, b = c["named"]["tie"]
    assert a < b and r["best1"][s] == a and r["dist1"][s] == 7
    assert not so.cells(c["kf2"])[2].all() and (r["best1"] >= 0).sum() >= 30
    fine = dict(c, kf2=dict(c["kf2"], grid=so.GRID_VGA))
    assert so.search(k1, fine, "f64", tgt1=so.target_1())["best1"][s] == b
