"""CPU: the conditions on tests/search_sim3_oracle.py under which tests/test_gpu_search_sim3.py decides anything -- the two flavours
agree outside the band, at most 2 % of a candidate's source slots lie inside it, every edge case the kernel can go wrong at occurs
in the pool, and the brute-force form with the 64-bit key (what csrc/search_sim3.hpp computes) equals the literal grid walk."""
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
