"""CPU: the fixtures of tests/search_triangulation_oracle.py reach every branch of ORBmatcher::SearchForTriangulation, and the closed
form -- the argmin of (distance, -position) over the passing targets -- equals the literal serial loop on every one of them."""
import numpy as np

from tests import search_triangulation_oracle as to

f32 = np.float32


def hand(only_stereo=0, ori=0):
    return to.expected("hand", only_stereo, ori)[0], to.hand_pair().named


def test_every_branch_is_reached():
    total = dict.fromkeys(to.BRANCHES, 0)
    for name in to.scenes():
        for only_stereo, ori in to.MODES:
            for r in to.expected(name, only_stereo, ori):
                for k, v in r["count"].items():
                    total[k] += v
    print(total)
    for k in to.BRANCHES:
        assert total[k] > 0, k
    # the random pool alone reaches the everyday ones
    pool = dict.fromkeys(to.BRANCHES, 0)
    for only_stereo, ori in to.MODES:
        for r in to.expected("pool", only_stereo, ori):
            for k, v in r["count"].items():
                pool[k] += v
    for k in ("matched", "epipole_not_applied", "line_refused", "dist_eq_th_accepted", "dist_th_plus_1_refused", "only_stereo_source",
              "only_stereo_target", "node_one_sided", "no_eligible_target"):
        assert pool[k] > 0, k


def test_the_hand_cases_decide_as_designed():
    r, nd = hand()
    raw, dist = r["match_raw"], r["dist"]
    assert raw[nd["d49"]] == nd["d49_t"][0] and dist[nd["d49"]] == 49
    assert raw[nd["d50"]] == nd["d50_t"][0] and dist[nd["d50"]] == 50           # the bound is inclusive
    assert raw[nd["d51"]] == -1 and dist[nd["d51"]] == -1
    assert raw[nd["equal_later_replaces"]] == nd["equal_later_replaces_t"][1]     # an equal distance later in the list replaces
    assert raw[nd["equal_zero"]] == nd["equal_zero_t"][2]
    # a target that fails a geometric test never changes the state, wherever it stands
    assert raw[nd["nearer_fails_line"]] == nd["nearer_fails_line_t"][1] and dist[nd["nearer_fails_line"]] == 20
    assert raw[nd["nearer_fails_line_after"]] == nd["nearer_fails_line_after_t"][0] and dist[nd["nearer_fails_line_after"]] == 20
    assert raw[nd["all_fail_line"]] == -1 and raw[nd["den_zero"]] == -1 and r["count"]["den_zero"] == 1
    # the epipole test needs BOTH sides mono
    assert raw[nd["epipole_mono_mono"]] == -1
    assert raw[nd["epipole_mono_stereo"]] == nd["epipole_mono_stereo_t"][0] and raw[nd["epipole_stereo_mono"]] == nd["epipole_stereo_mono_t"][0]
    assert raw[nd["epipole_level1"]] == -1 and raw[nd["epipole_level0"]] == nd["epipole_level0_t"][0]       # 100 * the TARGET's scale factor
    assert r["count"]["epipole_skip"] == 2
    assert raw[nd["no_eligible_target"]] == -1 and raw[nd["source_not_eligible"]] == -1
    # equal minima on one lane residue (positions 3 and 67) and on two (5 and 9): the later wins
    assert raw[nd["tie_lane"]] == nd["tie_lane_second"] and r["ties"][nd["tie_lane"]] == [3, 67]
    assert raw[nd["tie_lanes"]] == nd["tie_lanes_second"] and r["ties"][nd["tie_lanes"]] == [5, 9]
    # vbMatched2 is never set: two sources share a target
    assert raw[nd["share_a"]] == raw[nd["share_b"]] == nd["share_t"] and (dist[nd["share_a"]], dist[nd["share_b"]]) == (2, 6)
    assert r["count"]["empty_node"] == 2 and r["count"]["node_one_sided"] >= 4
    # only_stereo skips on either side
    s, _ = hand(only_stereo=1)
    assert raw[nd["mono_pair_far_from_epipole"]] >= 0 and s["match_raw"][nd["mono_pair_far_from_epipole"]] == -1
    t = nd["stereo_source_mono_target_t"]
    assert raw[nd["stereo_source_mono_target"]] == t[0] and s["match_raw"][nd["stereo_source_mono_target"]] == t[1]
    assert s["count"]["only_stereo_source"] > 0 and s["count"]["only_stereo_target"] > 0


def test_dsqr_on_both_sides_of_the_double_threshold():
    """The search of threshold_pairs finds, per level, a key-point pair whose dsqr is the largest float32 below the DOUBLE
    3.84 * sigma2 and one whose dsqr is the next float32.  On levels 0, 1 and 2 the product rounds DOWN to float32, so
    dsqr == (float)(3.84 * sigma2) is accepted by the reference's double compare and would be refused by a float32 compare: level 0
    pins that value.  On level 3 the product rounds up and both compares agree; the nearest pair is pinned there."""
    r, nd = hand()
    differs = 0
    for level in to.THRESHOLD_LEVELS:
        P = to.threshold_pairs(level)
        T = 3.84 * float(to.SIGMA2[level])
        for side, accepted in (("below", True), ("at_or_above", False)):
            y1, y2, want = P[side]
            assert to._dsqr_hand(y1, y2) == want and type(want) is f32
            ok, dsqr = to.check_dist_epipolar_line(np.array([100, y1], f32), np.array([100, y2], f32), to.F_HAND, to.SIGMA2[level],
                                                   dict(den_zero=0))
            assert dsqr == want and ok == accepted == (float(want) < T)
            src = nd["thr_%d_%s" % (level, side)]
            assert r["match_raw"][src] == (nd["thr_%d_%s_t" % (level, side)] if accepted else -1)
        assert np.nextafter(P["below"][2], f32(np.inf)) == P["at_or_above"][2]
        if P["float_compare_differs_at"] is not None:
            v = P["float_compare_differs_at"]
            assert v == P["below"][2] == f32(T) and float(v) < T and not (v < f32(T))
            differs += 1
    assert differs >= 1 and to.threshold_pairs(3)["float_compare_differs_at"] is None


def test_non_finite_values_never_match_and_never_skip():
    shared, cands, F12, exy = to.scenes()["pool"]
    assert np.isnan(F12[to.POOL_NAN_F]).any() and np.isnan(exy[to.POOL_NAN_E]).any() and np.isinf(cands[to.POOL_INF_KP]["xy"]).any()
    full = to.expected("pool", 0, 0)
    assert full[0]["n_matches"] > 0 and full[to.POOL_NAN_F]["n_matches"] == 0            # a NaN line never passes
    # a NaN epipole skips nothing: every mono pair goes on to the line test
    assert full[to.POOL_NAN_E]["count"]["epipole_skip"] == 0 and full[to.POOL_NAN_E]["n_matches"] >= full[1]["n_matches"] > 0
    bad = np.flatnonzero(np.isinf(cands[to.POOL_INF_KP]["xy"][:, 0]))
    assert not np.isin(full[to.POOL_INF_KP]["match_raw"], bad).any() and full[to.POOL_INF_KP]["n_matches"] > 0
    assert full[to.POOL_EMPTY]["n_matches"] == 0


def test_lengths_fixture():
    r, nd = to.expected("lengths", 0, 0)[0], to.lengths_pair().named
    for n_t in to.LENGTHS:
        ends, first, tgt = nd["ends_%d" % n_t], nd["first_%d" % n_t], nd["targets_%d" % n_t]
        assert len(tgt) == n_t
        if n_t == 0:
            assert r["match_raw"][ends] == -1 and r["match_raw"][first] == -1
        else:
            assert r["match_raw"][ends] == tgt[-1] and r["match_raw"][first] == tgt[0] and r["dist"][ends] == 6 and r["dist"][first] == 4
            assert r["ties"][ends] == ([0, n_t - 1] if n_t > 1 else [0])
    B = to.big_pair(4097)
    w = to.literal(B.frame(0), B.frame(1), to.F_HAND, to.E_HAND)
    assert w["match_raw"][B.named["src"]] == B.named["last"] and w["dist"][B.named["src"]] == 9 and w["ties"][B.named["src"]] == [0, 4096]


def test_closed_form_equals_the_literal_loop():
    for name, (shared, cands, F12, exy) in to.scenes().items():
        for only_stereo in (0, 1):
            for i, c in enumerate(cands):
                raw, dist = to.closed_form(shared, c, F12[i], exy[i], only_stereo=bool(only_stereo))
                want = to.expected(name, only_stereo, 0)[i]
                assert np.array_equal(raw, want["match_raw"]) and np.array_equal(dist, want["dist"]), (name, only_stereo, i)
                assert want["pairs"] == [(j, int(m)) for j, m in enumerate(want["match"]) if m >= 0]


def test_the_orientation_tail_culls():
    culled = 0
    for name in ("pool", "hand"):
        for a, b in zip(to.expected(name, 0, 0), to.expected(name, 0, 1)):
            assert np.array_equal(a["match_raw"], b["match_raw"]) and a["hist"].sum() == 0 and list(a["ind"]) == [-1, -1, -1]
            assert b["hist"].sum() == (b["match_raw"] >= 0).sum()
            culled += a["n_matches"] - b["n_matches"]
    assert culled > 0
