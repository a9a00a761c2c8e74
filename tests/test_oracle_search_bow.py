"""CPU: the two restatements of tests/search_bow_oracle.py agree bit for bit on every fixture in both modes, every fixture does
what it is for, and the hand-made cases decide what they were made to decide (tests/test_gpu_search_bow.py holds the device to
the literal restatement on the same fixtures)."""
import numpy as np
import pytest

from tests import search_bow_oracle as bo

f32 = np.float32


def runs():
    for name, (shared, cands, sis) in bo.scenes().items():
        for pi, p in enumerate(bo.params_of(name)):
            for ori in (1, 0):
                yield name, pi, ori, shared, cands, sis, p


def test_the_two_restatements_agree_bit_for_bit():
    n = 0
    for name, pi, ori, shared, cands, sis, p in runs():
        for k, (c, a) in enumerate(zip(cands, bo.expected(name, pi, ori))):
            b = bo.by_sets(shared, c, shared_is_source=sis, check_orientation=bool(ori), **p)
            assert bo.same(a, b), (name, pi, ori, k)
            n += 1
    assert n >= 60
    assert max(len(f["angle"]) for s, c, _ in bo.scenes().values() for f in [s] + c) <= 330      # "about 300": the six target lists of the lengths fixture sum to 323
    assert max(len(c) for _, c, _ in bo.scenes().values()) <= 8


@pytest.mark.parametrize("mode", ["kf", "frame"])
def test_every_fixture_does_what_it_is_for(mode):
    B = bo.steal_nodes(0)
    r = bo.expected(mode + "_steal", 0, 1)[0]
    a, b = B.named["A"], B.named["B"]
    # 1. B loses its nearest target (A', 12 away) to the earlier A and takes B'' (20 away)
    assert r["match_raw"][a] == B.named["A'"] and r["dist"][a] == 3
    assert r["match_raw"][b] == B.named["B''"] and r["dist"][b] == 20 and r["info"][b]["stolen"]
    assert bo.hamming(B.d[0][b], B.d[1][B.named["A'"]]) == 12
    B = bo.steal_nodes(1)
    r = bo.expected(mode + "_steal_ratio", 0, 1)[0]
    i = r["info"][B.named["B"]]                                         # ... and with a third target 24 away fails the ratio test
    assert (i["best1"], i["best2"], i["stolen"], i["under"], i["ok"]) == (20, 24, True, True, False) and r["match_raw"][B.named["B"]] == -1
    pool = [bo.expected(mode + "_pool", 0, 1)[k] for k in range(8)]
    assert sum(x["info"][s]["stolen"] and x["info"][s]["ok"] for x in pool for s in x["info"]) >= 1      # seeded frames do it too
    # 2. a rotation cull removes matches; one candidate keeps all three bins
    assert any(0 < x["n_matches"] < int((x["match_raw"] >= 0).sum()) for x in pool)
    assert any((x["ind"] >= 0).all() and x["hist"][x["ind"]].min() > 0 for x in pool)
    # 3. max2 < 0.1 max1
    r = bo.expected(mode + "_small_max2", 0, 1)[0]
    assert list(r["ind"]) == [4, -1, -1] and sorted(r["hist"])[-2:] == [3, 31] and f32(3) < f32(0.1) * f32(31)
    assert r["n_matches"] == 31 and int((r["match_raw"] >= 0).sum()) == 36
    # 4. equal bin counts: the earlier bin wins under the strict >
    r = bo.expected(mode + "_equal_bins", 0, 1)[0]
    assert list(r["hist"][[2, 5, 7, 9, 11]]) == [6, 6, 6, 6, 2] and list(r["ind"]) == [2, 5, 7] and r["n_matches"] == 18
    # without the orientation check nothing is culled and the histogram stays empty
    r0 = bo.expected(mode + "_equal_bins", 0, 0)[0]
    assert r0["n_matches"] == 26 and not r0["hist"].any() and list(r0["ind"]) == [-1, -1, -1]
    assert np.array_equal(r0["match"], r0["match_raw"]) and np.array_equal(r0["match_raw"], r["match_raw"])


def test_degenerate_frames():
    sc = bo.scenes()
    assert not sc["kf_source_not_eligible"][0]["eligible"].any() and len(sc["kf_source_empty"][0]["angle"]) == 0
    for name in ("kf_source_not_eligible", "kf_source_empty", "frame_target_empty"):
        assert all(r["n_matches"] == 0 and (r["match_raw"] == -1).all() for r in bo.expected(name, 0, 1))
    s, c, _ = sc["frame_pool"]
    assert s["eligible"] is None and len(c[1]["angle"]) == 0 and not c[3]["eligible"].any() and len(c[3]["angle"]) == 100
    r = bo.expected("frame_pool", 0, 1)
    assert r[1]["n_matches"] == 0 and len(r[1]["match"]) == 0 and r[3]["n_matches"] == 0
    s, c, _ = sc["kf_pool"]
    assert len(c[0]["angle"]) == 0 and not c[4]["eligible"].any() and len(c[5]["angle"]) > 250
    # absent nodes: the walk skips ids only one side holds, at the start, in the middle and at the end
    ids_s, ids_t = set(s["node_id"].tolist()), set(c[6]["node_id"].tolist())
    assert ids_s - ids_t and ids_s & ids_t


@pytest.mark.parametrize("mode", ["kf", "frame"])
def test_target_list_lengths(mode):
    B = bo.lengths_pair()
    tgt = B.frame(1)
    assert list(np.diff(tgt["node_off"])) == [0, 1, 63, 64, 65, 130]
    r = bo.expected(mode + "_lengths", 0, 0)[0]
    src = B.frame(0)
    for k, n_t in enumerate((0, 1, 63, 64, 65, 130)):
        first, second, third = src["feat"][3 * k:3 * k + 3]
        last = tgt["feat"][tgt["node_off"][k + 1] - 1] if n_t else -1
        assert r["match_raw"][first] == last and r["match_raw"][third] == -1, n_t           # the target at the END of the list
        if n_t > 1:                                                                         # the second source takes the list's first
            assert r["match_raw"][second] == tgt["feat"][tgt["node_off"][k]] and r["dist"][second] == 34 and r["info"][second]["stolen"]
        else:
            assert r["match_raw"][second] == -1


@pytest.mark.parametrize("mode", ["kf", "frame"])
def test_the_hand_made_cases(mode):
    B = bo.hand_pair()
    n = B.named
    strict, incl, loose = (bo.expected(mode + "_hand", pi, 0)[0] for pi in range(3))
    hit = lambda r, name: int(r["match_raw"][n[name]])
    # 49 / 50 under the strict threshold, 50 / 51 under the inclusive one
    assert hit(strict, "d49") >= 0 and hit(strict, "d50") == -1 and hit(strict, "d51") == -1
    assert hit(incl, "d49") >= 0 and hit(incl, "d50") >= 0 and hit(incl, "d51") == -1
    assert strict["dist"][n["d49"]] == 49 and incl["dist"][n["d50"]] == 50
    for r in (strict, incl):
        i = r["info"][n["r30_40"]]
        assert (i["best1"], i["best2"]) == (30, 40) and hit(r, "r30_40") == -1 and not f32(30) < f32(0.75) * f32(40)
        for name, d in (("equal_minima", 10), ("equal_zero", 0)):      # two equal minima: bestDist2 == bestDist1, no match
            i = r["info"][n[name]]
            assert (i["best1"], i["best2"]) == (d, d) and hit(r, name) == -1
        i = r["info"][n["single"]]                                     # a single target: bestDist2 stays 256
        assert (i["best1"], i["best2"]) == (49, 256) and hit(r, "single") == n["single_t"][0]
    # ties (visible with nn_ratio above 1): the earlier list position wins, in one lane (p, p + 64) and across lanes
    tgt = B.frame(1)
    pos = {int(x): k for k, x in enumerate(tgt["feat"])}
    assert pos[n["tie_lane_second"]] - pos[n["tie_lane_first"]] == 64
    assert 0 < pos[n["tie_lanes_second"]] - pos[n["tie_lanes_first"]] < 64
    assert n["tie_lanes_first"] < n["tie_lanes_second"]
    for name in ("tie_lane", "tie_lanes"):
        i = loose["info"][n[name]]
        assert (i["best1"], i["best2"]) == (10, 10) and hit(loose, name) == n[name + "_first"] and hit(strict, name) == -1
    # with the ratio above 1 two equal minima DO match, the first of the two -- but never at distance 0 (0 < 1.5 * 0 is false)
    assert hit(loose, "equal_minima") == n["equal_minima_t"][0] and hit(loose, "equal_zero") == -1
    # a feat list that is not ascending: the listed order decides
    src = B.frame(0)
    lst = src["feat"][src["node_off"][list(src["node_id"]).index(22)]:][:2]
    assert list(lst) == [n["unsorted_early"], n["unsorted_late"]] and lst[0] > lst[1]
    assert hit(strict, "unsorted_early") == n["unsorted_t"] and hit(strict, "unsorted_late") == -1
    # nodes only one frame holds: at the start, in the middle and at the end of the walk
    ids_s, ids_t = list(src["node_id"]), list(tgt["node_id"])
    assert ids_s[0] == 1 and ids_t[0] == 2 and 11 in ids_s and 12 in ids_t and 13 in ids_t and ids_s[-1] == 90 and ids_t[-1] == 95
    assert not {1, 11, 90} & set(ids_t) and not {2, 12, 13, 95} & set(ids_s)
    # the angles
    ang = lambda name: (src["angle"][n[name]], tgt["angle"][n[name + "_t"][0]])
    assert bo.rot_bin(*ang("rot_negative")) == 1 and ang("rot_negative")[0] - ang("rot_negative")[1] < 0
    assert bo.rot_bin(*ang("rot_zero")) == 0
    a, b = ang("rot_minus_zero")
    assert np.signbit(a) and np.signbit(f32(a) - f32(b)) and bo.rot_bin(a, b) == 0
    a, b = ang("rot_wraps_to_360")
    assert f32(a) - f32(b) < 0 and f32((f32(a) - f32(b)) + f32(360.0)) == f32(360.0) and bo.rot_bin(a, b) == 12
    a, b = ang("rot_half")
    v = float(f32(f32(a) * bo.FACTOR))
    assert v - np.floor(v) == 0.5 and bo.rot_bin(a, b) == int(v + 0.5) and int(np.round(v)) != bo.rot_bin(a, b)   # np.round would differ
    with_ori = bo.expected(mode + "_hand", 0, 1)[0]
    for name, b_ in (("rot_negative", 1), ("rot_zero", 0), ("rot_minus_zero", 0), ("rot_wraps_to_360", 12), ("rot_half", bo.rot_bin(*ang("rot_half")))):
        assert hit(with_ori, name) >= 0 and with_ori["hist"][b_] >= 1
    assert with_ori["hist"][13:].sum() == 0                            # rot * (1.0f / 30) never leaves [0, 12]
