"""The call sequences of tests/ba_sequences.py driven through the C oracle on the CPU: each must reach what it is meant to reach,
so that tests/test_gpu_ba_reuse.py (the same sequences on a reused GPU problem) cannot pass vacuously.  The bands below are
conditions on the scenes, not tolerances on a result."""
import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import ba_sequences as seq


def _records(name, op):
    recs, _ = seq.oracle_run(name)
    return [r for st, r in zip(seq.SEQUENCES[name][1], recs) if st[0] == op]


def _level1_fraction(levels):
    n1 = sum(int(np.count_nonzero(a)) for a in levels)
    return n1 / float(sum(len(a) for a in levels))


@pytest.mark.parametrize("name", ["A", "D", "S2"])
def test_a_local_joint_leaves_an_outlier_set_worth_losing(name):
    """between 1 % and 50 % of the edges are at level 1 after the local BA on the device-boundary, host-boundary and sharded scenes"""
    steps = seq.SEQUENCES[name][1]
    _, levels = seq.oracle_run(name)
    frac = _level1_fraction(levels[steps.index(seq.LJ)])
    assert 0.01 <= frac <= 0.50, frac


def test_boundary_scenes_take_the_path_they_are_named_after():
    """what qsp_ba_local_joint needs for its device-side stage boundary, read off the oracle's run: the device scene has it, the
    host scene loses object 0 (and only it) at the boundary, and the sharded scene has it as well (S2 runs on it)"""
    dev, host, sh = _records("A", "local_joint")[0], _records("D", "local_joint")[0], _records("S2", "local_joint")[0]
    assert seq.takes_device_boundary(dev)
    assert not seq.takes_device_boundary(host)
    assert (host["t1"]["obj_hidx"] >= 0).all() and host["t2"]["obj_hidx"][0] < 0 and (host["t2"]["obj_hidx"][1:] >= 0).all()
    assert seq.takes_device_boundary(sh)
    # the second local BA of D starts from all-active levels again and drops object 0 again
    again = _records("D", "local_joint")[1]
    assert np.array_equal(again["t1"]["obj_hidx"], host["t1"]["obj_hidx"]) and again["t2"]["obj_hidx"][0] < 0


@pytest.mark.parametrize("name", ["A", "S2"])
def test_the_solve_after_a_local_joint_moves_and_needs_the_outlier_set(name):
    """optimize(3, Huber) right after a local BA: at least one accepted trial, and on all-active levels its first chi2 would be
    off by far more than the 1e-8 the GPU is held to -- a lost outlier set cannot hide inside the bar"""
    sname, steps = seq.SEQUENCES[name]
    t = _records(name, "optimize")[0]["t"]
    assert int(np.sum(t["accepted"])) >= 1
    sc = seq.scene(sname)
    lost = bo.BaProblem(sc)
    lost.local_joint_ba()
    lost.set_levels(None, None, None)
    u = lost.optimize(*steps[[s[0] for s in steps].index("optimize")][1:])
    assert abs(u["chi2"][0] - t["chi2"][0]) > 1e-3 * abs(t["chi2"][0]), (u["chi2"][0], t["chi2"][0])
    if name == "A":      # ... and on this scene the outliers take landmarks out of the index: get_index has something to say too
        assert not np.array_equal(u["pt_hidx"], t["pt_hidx"])
    else:                # S2: landmarks of BOTH ranks stay in the index, so another rank's ownership mask in the levels would show
        act = sc["pt_id"][t["pt_hidx"] >= 0] % 2
        assert (act == 0).sum() > 50 and (act == 1).sum() > 50


def test_sharding_before_the_first_solve_must_not_count_edges_twice():
    """S1: a rank that linearises every edge would report `world` times the chi2 (the camera-object edges, counted by rank 0
    alone, are a small part of it)"""
    sc = seq.scene("sharded")
    p = bo.BaProblem(sc)
    t = p.optimize(1, seq.DM, seq.DS, seq.DO)
    e = p.edges()
    assert e["oe_chi2"].sum() < 0.5 * (e["mono_chi2"].sum() + e["st_chi2"].sum())
    assert len(_records("S1", "optimize")[0]["t"]["chi2"]) >= 2 and t["chi2"][0] > 0


@pytest.mark.parametrize("name", ["C", "F"])
def test_custom_levels_drop_landmark_zero(name):
    sname, steps = seq.SEQUENCES[name]
    sc = seq.scene(sname)
    mono, stereo, _ = seq.custom_levels(sc)
    assert mono.sum() + stereo.sum() >= 2                     # (landmark 0 has edges to lose)
    opts = _records(name, "optimize")
    assert opts[0]["t"]["pt_hidx"][0] == -1 and (opts[0]["t"]["pt_hidx"][1:] >= 0).sum() > 0
    if name == "C":
        assert _records(name, "local_joint")[0]["t2"]["pt_hidx"][0] >= 0       # (it was active until the custom levels came)
    else:
        assert opts[1]["t"]["pt_hidx"][0] >= 0                # set_levels(None) brings it back: the all-active index
        # F's last solve is the first solve of a fresh problem
        fresh = bo.BaProblem(sc).optimize(*steps[-1][1:])
        assert np.array_equal(opts[1]["t"]["chi2"], fresh["chi2"]) and np.array_equal(opts[1]["t"]["pt_hidx"], fresh["pt_hidx"])
        assert not np.array_equal(opts[0]["t"]["chi2"], fresh["chi2"])


def test_object_elimination_has_something_to_eliminate():
    """E toggles QSP_BA_OPT_OBJECT_ELIMINATION.  n_pose_blocks (free key-frames + objects, include/qsp_hip.h) does not depend on
    it; the size of the dense system does.  The library eliminates when there are active objects and every free key-frame comes
    before every object in the hessian order -- which the scene must offer, or both settings run the same code."""
    t1 = _records("E", "local_joint")[0]["t1"]
    kf, ob = t1["kf_hidx"], t1["obj_hidx"]
    n_free = int((kf >= 0).sum())
    assert n_free > 0 and (ob >= 0).sum() > 0 and kf.max() == n_free - 1 and ob[ob >= 0].min() == n_free
    runs = _records("E", "local_joint")
    assert len(runs) == 3
    for r in runs[1:]:                                        # the oracle knows no such option: three identical runs
        assert np.array_equal(r["t2"]["chi2"], runs[0]["t2"]["chi2"])


def test_a_stopped_local_joint_touches_nothing():
    """H: with the stop flag up at the call, the oracle (like src/Optimizer_util.cc:588-595) returns before anything is set up"""
    sc = seq.scene("sharded")
    stopped, full = _records("H", "local_joint_stopped")[0], _records("H", "local_joint")[0]
    for a, b in zip(stopped["state"], (sc["kf_pose"], sc["pt_xyz"], sc["obj_pose"])):
        assert np.array_equal(a, b)
    fresh = bo.BaProblem(sc)
    f1, f2 = fresh.local_joint_ba()
    assert np.array_equal(full["t2"]["chi2"], f2["chi2"]) and int(np.sum(full["t1"]["accepted"])) >= 1


@pytest.mark.parametrize("name", sorted(seq.SEQUENCES))
def test_solver_options_are_invisible_to_the_oracle_and_every_solve_iterates(name):
    """every solve of every sequence records at least one iteration, and the steps the oracle skips are solver options only"""
    sname, steps = seq.SEQUENCES[name]
    recs, levels = seq.oracle_run(name)
    assert len(recs) == len(steps) == len(levels)
    for st, r in zip(steps, recs):
        if st[0] in seq.SOLVER_OPTIONS:
            assert r is None
        elif st[0] == "local_joint":
            assert len(r["t1"]["chi2"]) >= 1 and len(r["t2"]["chi2"]) >= 1
        elif st[0] == "optimize":
            assert len(r["t"]["chi2"]) >= 1
