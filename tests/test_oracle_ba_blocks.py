"""CPU: the scene table of tests/ba_block_scenes.py is what it claims to be, and the C oracle is a sharp reference at these sizes.
Every scene's dense dimension, padded dimension, block rows, padding and side of the split threshold are computed from the index
tables of an oracle run and asserted against the table for both object-elimination settings; the oracle's two solvers (dense
Cholesky, block-sparse Cholesky in minimum-degree order) walk the same Levenberg-Marquardt path, accept every iteration at its
first trial (the scenes are there to test the linear solve, not LM's branching) and agree to a quarter of the 1e-8 bar the GPU
test holds the device solve to.  Run with -s for the table."""
import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import ba_block_scenes as bs

SENSITIVITY_BAR = 2.5e-9              # one quarter of the project's 1e-8 parity bar: the bar can discriminate


def _run(sc, sparse, n_iter, deltas):
    bo.set_sparse_solver(sparse)
    try:
        p = bo.BaProblem(sc)
        t = p.optimize(n_iter, *deltas)
    finally:
        bo.set_sparse_solver(0)
    return t, p.state()


def _distance(ta, sa, tb, sb):
    """the largest relative distance of two oracle runs in chi2, lambda and the three state arrays (the GPU test's measures)"""
    d = [bs.rel(ta["chi2"], tb["chi2"], 1e-8, 1e-12), bs.rel(ta["lam"], tb["lam"], 1e-8, 1e-12)]
    d += [bs.rel(x, y, 1e-8, 1e-10) for x, y in zip(sa, sb)]
    return max(d)


def test_ticket_scene_derivation():
    assert bs.ticket_nb(256) == (24, False)
    e = bs.entry("b_ticket", 256)
    assert (e["n_kf"], e["elim"]) == (257, (1536, 1536))
    for n_cu in (64, 104, 120, 228, 256, 304):
        nb, capped = bs.ticket_nb(n_cu)
        assert not capped and nb * (nb - 1) // 2 > n_cu - 1 >= (nb - 1) * (nb - 2) // 2
        e = bs.entry("b_ticket", n_cu)
        assert e["elim"][1] == bs.NB * nb and bs.shape(e["n_kf"] - 1, bs.N_OBJ, True).split
    assert bs.ticket_nb(512) == (bs.NB_TICKET_CAP, True)          # 465 tiles at 31 block rows do not exceed 511 workgroups


@pytest.mark.parametrize("name", bs.NAMES)
def test_scene_is_what_the_table_says_and_the_oracle_is_sharp_there(name):
    e = bs.entry(name)
    sc = bs.scene(name)
    deltas = (bs.DM, bs.DS, bs.DO)
    ts, ss = _run(sc, 1, 2, deltas)
    # ---- scene shape, from the index tables of the oracle run
    kh, oh = ts["kf_hidx"], ts["obj_hidx"]
    n_free, n_obj = int((kh >= 0).sum()), int((oh >= 0).sum())
    assert n_free == e["n_kf"] - 1 and n_obj == bs.N_OBJ
    assert int(kh.max()) == n_free - 1 and int(oh.min()) == n_free          # key-frames in front of the objects: elimination applies
    assert (ts["pt_hidx"] >= 0).all()
    obs = np.bincount(sc["mono_kf"], minlength=e["n_kf"])
    assert obs[kh >= 0].min() >= 6, "a free key-frame with fewer than 6 observations"
    se, sj = bs.shape(n_free, n_obj, True), bs.shape(n_free, n_obj, False)
    assert (se.dim, se.dimp) == e["elim"] and (sj.dim, sj.dimp) == e["joint"]
    want = dict(b1=(1, 4, True), b2=(2, 62, True), b3_exact=(3, 0, True), b4_pad=(4, 58, True), b6_exact=(6, 0, True),
                b18_exact=(18, 0, True), b_ticket=(24, 0, True), b31=(31, 4, True), b32=(32, 2, False))[name]
    assert (se.nb, se.pad, se.split) == want
    assert se.split == (se.dimp <= 1984) and sj.split == (sj.dimp <= 1984)
    if name == "b3_exact":
        assert (sj.dim, sj.dimp, sj.pad) == (210, 256, 46)                  # the padded case with objects inside
    if name == "b_ticket":
        assert se.nb * (se.nb - 1) // 2 > bs.N_CU_CPU - 1
    # ---- oracle runs: every iteration accepted at its first trial, dense and sparse solver on the same path
    assert list(ts["trials"]) == [1, 1] and list(ts["accepted"]) == [1, 1] and ts["iterations"] == 2
    assert ts["chi2"][1] < ts["chi2"][0]
    t1, s1 = _run(sc, 1, 1, (0.0, 0.0, 0.0))                                # the one-step run without a robust kernel
    assert list(t1["trials"]) == [1] and list(t1["accepted"]) == [1]
    dist = None
    if name in bs.DENSE_ORACLE:
        td, sd = _run(sc, 0, 2, deltas)
        assert list(td["trials"]) == list(ts["trials"]) and list(td["accepted"]) == list(ts["accepted"])
        assert td["result"] == ts["result"] and td["iterations"] == ts["iterations"]
        u1, r1 = _run(sc, 0, 1, (0.0, 0.0, 0.0))
        assert list(u1["trials"]) == list(t1["trials"]) and list(u1["accepted"]) == list(t1["accepted"])
        dist = max(_distance(td, sd, ts, ss), _distance(u1, r1, t1, s1))
    print("\n%-10s kf %3d  pts %4d  obs/kf >= %2d | elim: dim %4d dimp %4d nb %2d pad %2d %-9s | joint: dim %4d dimp %4d nb %2d pad %2d %-9s"
          " | dense-sparse %s | %s"
          % (name, e["n_kf"], e["n_pt"], obs[kh >= 0].min(), se.dim, se.dimp, se.nb, se.pad, "split" if se.split else "non-split",
             sj.dim, sj.dimp, sj.nb, sj.pad, "split" if sj.split else "non-split",
             "%.1e" % dist if dist is not None else "(sparse only)", e["regime"]))
    if dist is not None:
        assert dist <= SENSITIVITY_BAR, dist
