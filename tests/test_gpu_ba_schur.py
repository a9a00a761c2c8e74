"""GPU: the three forms of the bundle adjustment's Schur complement against the C oracle, one scene per regime of the dispatch in
the trial loop of qsp_ba_optimize (tests/ba_schur_scenes.py): the last size of k_schur_points and the first of k_schur_rows, block
rows with stereo edges and objects (eliminated behind them, or inside the dense system), block rows over the level-1 edges and the
inactive landmarks of a local joint BA's second stage, the largest row block that fits the LDS and the first that does not, graphs
above the pair-list cap in their default mode, and both piece lengths of the edge split.  qsp_ba_stats.schur_form says which form
the last trial took; every run asserts it, so a test cannot pass on another kernel than the one it names.
tests/test_oracle_ba_schur.py shows on the CPU that each scene is on its side of its threshold, that the oracle accepts every
iteration at its first trial there and that its two solvers agree to 1e-12, so the bars below measure the device code.

Bars (the ones test_atomic_schur_kernels_match_oracle holds for the atomic kernels): index tables, trial counts, accept flags, result
and iteration count exact; chi2 and lambda 1e-8 relative, lambda on the iterations whose chi2 still moves by more than 1e-3 of
itself; key-frames, points and objects 1e-7 relative / 1e-9 absolute.  Measured figures: profiles/ba_schur_margins.json.

Reference of rows_lds_last / rows_lds_over (3392 / 3456 unknowns): the ORACLE, with its block-sparse solver (5 to 16 s per scene on one
CPU core, once per session; its dense solver takes minutes there); the pair-list mode on the same graph is compared as well.

Every GPU configuration and every oracle run happens once per session (cached); the tests assert on those runs."""
import functools

import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import ba_schur_scenes as ss
from tests.margins import within

pytestmark = pytest.mark.gpu

DELTAS = (ss.DM, ss.DS, ss.DO)
PLAIN = (0.0, 0.0, 0.0)


def runs_of(name):
    """(key, iterations, Huber deltas) of the optimize calls of a scene, each from the initial state"""
    if name in ss.SPLIT:
        return (("2", 1, DELTAS),)
    return (("2", 2, DELTAS), ("1", 1, PLAIN))


def close(name, a, b, rtol=1e-8, atol=1e-12):
    """np.allclose(a, b, rtol, atol) with the measured effective relative error recorded under `name` (tests/margins.py)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    return within(name, ss.rel(a, b, rtol, atol), rtol) and bool(np.isfinite(a).all())


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle (block-sparse solver: the same answers as the dense one to 1e-12, tests/test_oracle_ba_schur.py) on the scene"""
    sc = ss.scene(name)
    out = {}
    bo.set_sparse_solver(1)
    try:
        if name == "rows_levels":
            p = bo.BaProblem(sc)
            out["j1"], out["j2"] = p.local_joint_ba()
            out["sj"], out["levels"] = p.state(), p.levels()
        else:
            for key, n_iter, deltas in runs_of(name):
                p = bo.BaProblem(sc)
                out["t" + key], out["s" + key] = p.optimize(n_iter, *deltas), p.state()
    finally:
        bo.set_sparse_solver(0)
    return out


def _configure(b, name, mode):
    """mode: `default` (no mode call), `atomic`, `atomic_joint` (objects inside the dense system), `pairs`, `refused` (pair lists
    asked for above the cap).  -> the form the next solve must take"""
    from qsp_slam_amd import _lib
    c = ss.counts(ss.scene(name))
    if mode == "default":
        return ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj)
    if mode == "refused":
        with pytest.raises(_lib.QspError) as e:
            b.set_deterministic(True)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED
        return ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj, True)
    b.set_deterministic(mode == "pairs")
    if mode == "atomic_joint":
        b.set_object_elimination(False)
    return ss.predict(c.n_edge, c.pairs, c.n_kf, c.n_free, c.n_obj, mode == "pairs", elimination=mode != "atomic_joint")


@functools.lru_cache(maxsize=None)
def gpu_run(name, mode):
    """a fresh problem per solve; asserts after each that the predicted form is the one that ran"""
    from qsp_slam_amd.ba import BaProblem
    sc = ss.scene(name)
    out = {}
    if name == "rows_levels":
        b = BaProblem(sc)
        try:
            assert b.schur_form == ss.NONE                       # nothing solved yet
            form = _configure(b, name, mode)
            out["j1"], out["j2"] = b.local_joint_ba()
            assert b.schur_form == form, (name, mode, b.schur_form, form)
            out["sj"], out["index"] = b.state(), b.index()
        finally:
            b.close()
        b = BaProblem(sc)                                        # the first stage alone: the edges' chi2 and depth signs at the stage boundary
        try:
            form = _configure(b, name, mode)
            out["stage1"] = b.optimize(5, *DELTAS)
            assert b.schur_form == form
            out["edges"] = b.edges()
        finally:
            b.close()
        return out
    for key, n_iter, deltas in runs_of(name):
        b = BaProblem(sc)
        try:
            form = _configure(b, name, mode)
            out["t" + key] = b.optimize(n_iter, *deltas)
            assert b.schur_form == form, (name, mode, key, b.schur_form, form)
            assert b.profile(False).schur_form == form           # (filled with profiling off)
            out["s" + key] = b.state()
        finally:
            b.close()
    return out


def same_trace(tag, tg, tr, index=True):
    """exact: index tables (a stage of local_joint_ba() carries none: index=False), trials, accept flags, result, iterations;
    1e-8: chi2, and lambda where chi2 still moves"""
    if index:
        assert np.array_equal(tg["kf_hidx"], tr["kf_hidx"]) and np.array_equal(tg["obj_hidx"], tr["obj_hidx"])
        assert np.array_equal(tg["pt_hidx"], tr["pt_hidx"])
    assert list(tg["trials"]) == list(tr["trials"]) and list(tg["accepted"]) == list(tr["accepted"])
    assert tg["result"] == tr["result"] and tg["iterations"] == tr["iterations"]
    m = ss.moving(tr["chi2"])
    ok = [close(tag + "chi2", tg["chi2"], tr["chi2"]), close(tag + "lam", np.asarray(tg["lam"])[m], np.asarray(tr["lam"])[m])]
    assert all(ok), (tag, ok)


def same_state(tag, sg, sr):
    ok = [close(tag + q, x, y, rtol=1e-7, atol=1e-9) for q, x, y in zip(("kf", "pt", "obj"), sg, sr)]
    assert all(ok), (tag, ok)


def assert_matches(tag, name, g, r):
    for key, _, _ in runs_of(name):
        pre = "%s/%s" % (tag, "" if key == "2" else "step_")
        same_trace(pre, g["t" + key], r["t" + key])
        same_state(pre, g["s" + key], r["s" + key])


@pytest.mark.parametrize("name", ss.MID + ss.LDS + ss.SPLIT)
def test_atomic_schur_forms_match_oracle(name):
    """set_deterministic(False) on every scene but rows_levels: form 1 at points_last, rows_lds_over and cap_points, form 2 at the
    others (asserted in gpu_run).  Two robust iterations and one plain step from the initial state (the two 2^18-edge scenes: one
    robust iteration), against the oracle; chi2 decreased."""
    g, r = gpu_run(name, "atomic"), oracle_run(name)
    assert_matches("ba_schur/%s/atomic" % name, name, g, r)
    if name not in ss.SPLIT:
        assert float(g["t2"]["chi2"][1]) < float(g["t2"]["chi2"][0])
        n_obj = int((r["t2"]["obj_hidx"] >= 0).sum())
        c = ss.counts(ss.scene(name))
        assert g["t2"]["n_pose_blocks"] == c.n_free + n_obj


def test_block_rows_with_the_objects_inside_the_dense_system():
    """rows_mixed with the object elimination off: k_schur_prepare lays the objects' blocks into Hs, k_schur_rows adds the
    key-frame rows beside them, no k_obj_rows"""
    assert_matches("ba_schur/rows_mixed/atomic_joint", "rows_mixed", gpu_run("rows_mixed", "atomic_joint"), oracle_run("rows_mixed"))


@pytest.mark.parametrize("name", ["rows_first", "rows_mixed"] + ss.LDS)
def test_pair_list_mode_on_the_same_graphs(name):
    """form 0 (asserted in gpu_run) against the oracle and against the atomic run: the same trial path, the same bars"""
    p, a = gpu_run(name, "pairs"), gpu_run(name, "atomic")
    assert_matches("ba_schur/%s/pairs" % name, name, p, oracle_run(name))
    assert_matches("ba_schur/%s/pairs_vs_atomic" % name, name, p, a)


@pytest.mark.parametrize("mode", ["atomic", "pairs"])
def test_second_stage_of_a_local_joint_ba(mode):
    """rows_levels through local_joint_ba(): the second stage runs over a graph with level-1 edges (k_schur_rows skips them on
    both sides of a pair), landmarks without an active edge (pt_h < 0) and landmarks with a single one.  Both stages against the
    oracle; the stage-2 index tables equal the oracle's; the outlier set that the device's first stage implies (chi2 above
    5.991 / 7.815 / 1e3 or a non-positive depth after optimize(5)) is exactly the oracle's."""
    g, r = gpu_run("rows_levels", mode), oracle_run("rows_levels")
    tag = "ba_schur/rows_levels/%s/" % mode
    same_trace(tag + "stage1_", g["j1"], r["j1"], index=False)
    same_trace(tag + "stage2_", g["j2"], r["j2"], index=False)        # (its index tables: just below)
    same_state(tag, g["sj"], r["sj"])
    for x, y in zip(g["index"], (r["j2"]["kf_hidx"], r["j2"]["obj_hidx"], r["j2"]["pt_hidx"])):
        assert np.array_equal(x, y)
    ph = g["index"][2]
    assert (ph < 0).any() and ph[ss.LOST_PT] < 0 and ph[ss.LONE_PT] >= 0
    assert g["j2"]["n_landmarks"] == int((r["j2"]["pt_hidx"] >= 0).sum()) < g["j1"]["n_landmarks"]
    same_trace(tag + "stage1_alone_", g["stage1"], r["j1"])
    e = g["edges"]
    assert np.array_equal((e["mono_chi2"] > 5.991) | ~e["mono_pos"], r["levels"][0] != 0)
    assert np.array_equal((e["st_chi2"] > 7.815) | ~e["st_pos"], r["levels"][1] != 0)
    assert np.array_equal(e["oe_chi2"] > 1e3, r["levels"][2] != 0)
    if mode == "pairs":
        a = gpu_run("rows_levels", "atomic")
        same_trace(tag + "vs_atomic_stage1_", g["j1"], a["j1"], index=False)
        same_trace(tag + "vs_atomic_stage2_", g["j2"], a["j2"], index=False)
        assert all(np.array_equal(x, y) for x, y in zip(g["index"], a["index"]))
        same_state(tag + "vs_atomic_", g["sj"], a["sj"])


@pytest.mark.parametrize("name", ss.CAP)
def test_graphs_above_the_pair_list_cap(name):
    """more than PAIR_CAP pair entries: a freshly created problem, with no mode call, runs the atomic kernels (form 1 at 28 200
    edges, form 2 at 66 000); set_deterministic(True) returns QSP_ERR_UNSUPPORTED and leaves the problem as it was -- the solve
    after it takes the same form and matches the oracle (all asserted in gpu_run / _configure)"""
    r = oracle_run(name)
    assert_matches("ba_schur/%s/default" % name, name, gpu_run(name, "default"), r)
    assert_matches("ba_schur/%s/refused" % name, name, gpu_run(name, "refused"), r)
