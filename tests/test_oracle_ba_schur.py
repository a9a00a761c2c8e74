"""CPU: the scene table of tests/ba_schur_scenes.py is what it claims to be, and the C oracle is a sharp reference there.  For every
scene: the form predict() gives from the counts, and the property that puts the scene on its side of a threshold (edge count, pair
count against the cap, free key-frames, dimp, LDS bytes of a row block against 160 KiB, piece length of the edge split); the oracle
accepts every iteration at its first trial, so no trial sequence can fork on rounding; the oracle's dense and block-sparse solvers
agree to 1e-12 on chi2 and states (not at the two 3392 / 3456-wide systems, where the dense solver takes minutes).  Run with -s for
the table."""
import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import ba_schur_scenes as ss

AGREE = 1e-12                         # dense against block-sparse solver, relative


def _run(sc, sparse, n_iter, deltas):
    bo.set_sparse_solver(sparse)
    try:
        p = bo.BaProblem(sc)
        t = p.optimize(n_iter, *deltas)
    finally:
        bo.set_sparse_solver(0)
    return t, p.state()


def _joint(sc, sparse):
    bo.set_sparse_solver(sparse)
    try:
        p = bo.BaProblem(sc)
        t1, t2 = p.local_joint_ba()
    finally:
        bo.set_sparse_solver(0)
    return t1, t2, p.state(), p.levels()


def _distance(ta, sa, tb, sb):
    """chi2 per iteration, relative; each state array relative to its largest entry (metres and unit quaternions: an entry near
    zero carries the absolute error of the sums it came from, it has no relative precision of its own)"""
    d = [ss.rel(ta["chi2"], tb["chi2"], AGREE, 1e-30)]
    d += [float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(sa, sb) if x.size]
    return max(d)


def test_prediction_restates_the_dispatch_rule():
    P = ss.predict
    assert P(65535, 1000, 9, 8, 0, False) == ss.POINTS and P(65536, 1000, 9, 8, 0, False) == ss.ROWS
    assert P(65536, 1000, 9, 8, 0) == ss.PAIRS and P(65536, 1000, 9, 8, 0, True) == ss.PAIRS
    assert P(100, ss.PAIR_CAP, 9, 8, 0) == ss.PAIRS and P(100, ss.PAIR_CAP + 1, 9, 8, 0) == ss.POINTS
    assert P(70000, ss.PAIR_CAP + 1, 9, 8, 0) == ss.ROWS and P(70000, ss.PAIR_CAP + 1, 9, 8, 0, True) == ss.ROWS     # refused: stays atomic
    assert P(70000, 1000, 4097, 8, 0) == ss.ROWS                                     # n_kf^2 > 2^24
    assert P(70000, 1000, 9, 0, 0) == ss.NONE and P(70000, 1000, 9, 0, 2, False) == ss.ROWS
    # the LDS edge: 565 free key-frames fit (with or without eliminated objects in front), 566 do not
    assert ss.dense_dimp(565, 3) == 3392 and ss.row_lds(3392) == 162864 <= ss.LDS_MAX < ss.row_lds(3456)
    assert ss.eliminated(565, 3) and not ss.eliminated(566, 3) and ss.dense_dimp(566, 3) == 3456
    assert ss.dense_dimp(565, 3, False) == 3456                                      # objects inside: already past the edge
    assert P(70000, 1000, 567, 565, 3, False) == ss.ROWS and P(70000, 1000, 568, 566, 3, False) == ss.POINTS
    assert P(70000, 1000, 567, 565, 3, False, elimination=False) == ss.POINTS
    assert ss.ksplit((1 << 18) - 1) == 512 and ss.ksplit(1 << 18) == 2048


@pytest.mark.parametrize("name", ss.NAMES)
def test_scene_is_what_the_table_says_and_the_oracle_is_sharp_there(name):
    s, sc = ss.TABLE[name], ss.scene(name)
    c = ss.counts(sc)
    dimp = ss.dense_dimp(c.n_free, c.n_obj)
    # ---- the regime, from counts
    assert c.n_edge == s.n_edge and c.n_obj == s.n_obj and c.n_free == s.n_kf - s.n_fixed
    assert ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj, False) == s.form
    assert int(np.asarray(sc["kf_fixed"]).sum()) == s.n_fixed >= 1
    fixed_seen = c.obs_per_kf[np.asarray(sc["kf_fixed"]) != 0]
    assert (fixed_seen > 0).all(), "a fixed key-frame without an edge would not reach the ha < 0 return"
    assert (c.obs_per_kf % 256 != 0).all()
    if s.obs < s.n_kf:
        assert len(np.unique(c.obs_per_kf)) >= min(s.n_kf, 8) - 1, "observation counts per key-frame are meant to be uneven"
    if name in ss.CAP:
        assert c.pairs > ss.PAIR_CAP and ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj) == s.form
        assert ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj, True) == s.form
        assert (c.n_edge >= ss.ROWS_MIN_EDGES) == (name == "cap_rows")
    else:
        assert c.pairs <= ss.PAIR_CAP and ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj) == ss.PAIRS
    if name == "points_last":
        assert c.n_edge == ss.ROWS_MIN_EDGES - 1
    if name == "rows_first":
        assert c.n_edge == ss.ROWS_MIN_EDGES and c.obs_per_kf.min() > 4 * ss.ksplit(c.n_edge)
    if name == "rows_mixed":
        assert len(sc["st_pt"]) > 0.25 * c.n_edge and len(sc["mono_pt"]) > 0.6 * c.n_edge and c.n_obj == 3
        assert ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj, False, elimination=False) == ss.ROWS
    if name == "rows_lds_last":
        assert c.n_free == 565 and dimp == 3392 and ss.eliminated(c.n_free, c.n_obj) and ss.row_lds(dimp) <= ss.LDS_MAX
        assert ss.row_lds(dimp + ss.NB) > ss.LDS_MAX and c.n_edge >= ss.ROWS_MIN_EDGES
    if name == "rows_lds_over":
        assert c.n_free == 566 and dimp == 3456 and not ss.eliminated(c.n_free, c.n_obj) and ss.row_lds(dimp) > ss.LDS_MAX
        assert c.n_edge >= ss.ROWS_MIN_EDGES
    if name == "cap_rows":
        assert (np.bincount(sc["mono_pt"]) == 300).all()
    if name == "split_small_last":
        assert c.n_edge == ss.KSPLIT_SMALL_BELOW - 1 and ss.ksplit(c.n_edge) == ss.KSPLIT_SMALL
    if name == "split_large_first":
        assert c.n_edge == ss.KSPLIT_SMALL_BELOW and ss.ksplit(c.n_edge) == ss.KSPLIT and c.obs_per_kf.min() > 4 * ss.KSPLIT
    # ---- the oracle: first-trial accepts, the index tables the counts promise, dense == sparse
    deltas = (ss.DM, ss.DS, ss.DO)
    dense = name not in ss.LDS
    dist = []
    if name == "rows_levels":
        t1, t2, st, lv = _joint(sc, 1)
        for t in (t1, t2):
            assert list(t["trials"]) == [1] * len(t["trials"]) and list(t["accepted"]) == [1] * len(t["trials"])
        ph = t2["pt_hidx"]
        active = np.bincount(np.concatenate([sc["mono_pt"][lv[0] == 0], sc["st_pt"][lv[1] == 0]]), minlength=len(ph))
        assert ph[ss.LOST_PT] < 0 and active[ss.LOST_PT] == 0 and t1["pt_hidx"][ss.LOST_PT] >= 0
        assert active[ss.LONE_PT] == 1 and ph[ss.LONE_PT] >= 0
        assert lv[0].sum() > 0.05 * len(lv[0]) and lv[1].sum() > 0.05 * len(lv[1])
        n_active = int((lv[0] == 0).sum() + (lv[1] == 0).sum())
        assert c.n_edge >= ss.ROWS_MIN_EDGES > n_active          # the rule counts every edge of the graph, level 1 included
        u1, u2, su, lu = _joint(sc, 0)
        assert all(np.array_equal(x, y) for x, y in zip(lv, lu))
        for t, u in ((t1, u1), (t2, u2)):
            assert list(t["trials"]) == list(u["trials"]) and t["result"] == u["result"]
        dist.append(max(_distance(t1, st, u1, su), _distance(t2, st, u2, su)))
        ts = t1
    else:
        n2 = 1 if name in ss.SPLIT else 2
        ts, st = _run(sc, 1, n2, deltas)
        assert list(ts["trials"]) == [1] * n2 and list(ts["accepted"]) == [1] * n2 and ts["iterations"] == n2
        assert n2 == 1 or ts["chi2"][1] < ts["chi2"][0]
        t1, s1 = _run(sc, 1, 1, (0.0, 0.0, 0.0))
        assert list(t1["trials"]) == [1] and list(t1["accepted"]) == [1]
        if dense:
            td, sd = _run(sc, 0, n2, deltas)
            u1, r1 = _run(sc, 0, 1, (0.0, 0.0, 0.0))
            assert list(td["trials"]) == list(ts["trials"]) and list(u1["trials"]) == list(t1["trials"])
            dist += [_distance(td, sd, ts, st), _distance(u1, r1, t1, s1)]
    kh, oh = ts["kf_hidx"], ts["obj_hidx"]
    assert int((kh >= 0).sum()) == c.n_free and int((oh >= 0).sum()) == c.n_obj
    assert int(kh.max()) == c.n_free - 1 and int(oh.min()) == c.n_free           # key-frames in front of the objects
    print("\n%-17s kf %3d (%d fixed)  edges %6d  pairs %8d  dimp %4d  row block %6d B  pieces of %4d  form %2d | dense-sparse %s | %s"
          % (name, c.n_kf, s.n_fixed, c.n_edge, c.pairs, dimp, ss.row_lds(dimp), ss.ksplit(c.n_edge), s.form,
             "%.1e" % max(dist) if dist else "(sparse only)", s.regime))
    if dist:
        assert max(dist) <= AGREE, dist
