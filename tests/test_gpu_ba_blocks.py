"""GPU: the dense solve of the bundle adjustment's reduced system against the C oracle at every block-row regime of the solver
(tests/ba_block_scenes.py: 1, 2, 3, 4, 6, 18 block rows, the first size at which a tile workgroup takes a second ticket, the last
size of the split back-substitution and the first of the other form; with and without padding rows), in both forms of the
factorisation (one launch with ticketed tile workgroups, one launch per block step) and with the objects eliminated in front of the
solve or inside it.  tests/test_oracle_ba_blocks.py shows on the CPU that every scene is what the table says and that the oracle's
two solvers agree to 1e-14 there, so the bars below -- the ones test_single_stage_matches_oracle holds -- measure the device code.

Every GPU configuration runs once per session (cached); the tests below assert on those runs."""
import functools

import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import ba_block_scenes as bs
from tests.margins import within

pytestmark = pytest.mark.gpu

FORMS = ["chain", "step"]
ELIMS = ["elim", "joint"]


@functools.lru_cache(maxsize=None)
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def close(name, a, b, rtol=1e-8, atol=1e-12):
    """np.allclose(a, b, rtol, atol) with the measured effective relative error recorded under `name` (tests/margins.py)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    return within(name, bs.rel(a, b, rtol, atol), rtol) and bool(np.isfinite(a).all())


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle (block-sparse solver) on the scene: optimize(2) with the Huber kernels and, from the initial state again,
    optimize(1) without.  Independent of every GPU option."""
    sc = bs.scene(name, n_cu())
    bo.set_sparse_solver(1)
    try:
        p = bo.BaProblem(sc)
        t2 = p.optimize(2, bs.DM, bs.DS, bs.DO)
        s2 = p.state()
        q = bo.BaProblem(sc)
        t1 = q.optimize(1, 0.0, 0.0, 0.0)
        s1 = q.state()
    finally:
        bo.set_sparse_solver(0)
    return dict(t2=t2, s2=s2, t1=t1, s1=s1)


def run_gpu(name, form, elim, deterministic=True):
    """a fresh problem per optimize call, in the asked-for configuration; asserts that this configuration is the one that ran"""
    from qsp_slam_amd.ba import BaProblem
    sc = bs.scene(name, n_cu())
    out = {}
    for key, n_iter, deltas in (("2", 2, (bs.DM, bs.DS, bs.DO)), ("1", 1, (0.0, 0.0, 0.0))):
        b = BaProblem(sc)
        try:
            b.set_deterministic(deterministic)
            b.set_object_elimination(elim == "elim")
            if form == "chain":
                assert b.cholesky_chain, "the chain form was not set up"
            else:
                b.set_cholesky_chain(False)
                assert not b.cholesky_chain
            t = b.optimize(n_iter, *deltas)
            prof = b.profile(False)
            if form == "chain":       # no flag wait expired and the problem is still on the chain form
                assert prof.chain_timeouts == 0 and prof.cholesky_chain == 1 and b.cholesky_chain
            else:
                assert prof.cholesky_chain == 0 and not b.cholesky_chain
            out["t" + key], out["s" + key] = t, b.state()
        finally:
            b.close()
    return out


gpu_run = functools.lru_cache(maxsize=None)(run_gpu)


def assert_matches_oracle(tag, g, r):
    for key, pre in (("2", ""), ("1", "step_")):
        tg, tr = g["t" + key], r["t" + key]
        assert np.array_equal(tg["kf_hidx"], tr["kf_hidx"]) and np.array_equal(tg["obj_hidx"], tr["obj_hidx"])
        assert np.array_equal(tg["pt_hidx"], tr["pt_hidx"])
        assert list(tg["trials"]) == list(tr["trials"]) and list(tg["accepted"]) == list(tr["accepted"])
        assert tg["result"] == tr["result"] and tg["iterations"] == tr["iterations"]
        ok = [close("%s/%schi2" % (tag, pre), tg["chi2"], tr["chi2"]), close("%s/%slam" % (tag, pre), tg["lam"], tr["lam"])]
        for q, x, y in zip(("kf", "pt", "obj"), g["s" + key], r["s" + key]):
            ok.append(close("%s/%s%s" % (tag, pre, q), x, y, rtol=1e-8, atol=1e-10))
        assert all(ok), (tag, key, ok)


def same_bits(a, b):
    for key in ("2", "1"):
        ta, tb = a["t" + key], b["t" + key]
        for q in ("chi2", "lam", "trials", "accepted"):
            assert np.array_equal(ta[q], tb[q]), (key, q)
        for x, y in zip(a["s" + key], b["s" + key]):
            assert np.array_equal(x, y), key


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", bs.NAMES)
def test_dense_solve_matches_oracle(name, form, elim):
    """(a) index tables, trials, accept flags, result and iteration count exact; chi2 and lambda to 1e-8; key-frames, points and
    objects to 1e-8 / 1e-10 -- after two robust iterations and after one plain step, whose state is exp(dx) T: a direct image of
    the solve's x.  (b) the dimension the solver saw is the table's."""
    e = bs.entry(name, n_cu())
    r = oracle_run(name)
    g = gpu_run(name, form, elim)
    n_obj = int((r["t2"]["obj_hidx"] >= 0).sum())
    for key in ("t2", "t1"):
        n_pose = int(g[key]["n_pose_blocks"])
        s = bs.shape(n_pose - n_obj, n_obj, elim == "elim")
        assert (s.dim, s.dimp) == e[elim], (name, elim, n_pose, s)
    if name == "b_ticket" and elim == "elim":
        nb, capped = bs.ticket_nb(n_cu())
        assert s.nb == nb
        if capped:
            print("b_ticket: capped at %d block rows, %d tiles do not exceed %d compute units" % (nb, nb * (nb - 1) // 2, n_cu()))
        else:
            assert nb * (nb - 1) // 2 > n_cu() - 1
    assert_matches_oracle("ba_blocks/%s/%s/%s" % (name, form, elim), g, r)


@pytest.mark.parametrize("elim", ELIMS)
@pytest.mark.parametrize("name", bs.NAMES)
def test_chain_and_step_forms_and_repeated_runs_give_the_same_bits(name, elim):
    """(c) test_cholesky_chain_and_step_forms_give_the_same_bits (tests/test_gpu_ba.py: 2, 5 and 19 block rows) at every regime of
    the table, and a second run of the chain form against the first"""
    chain = gpu_run(name, "chain", elim)
    same_bits(chain, gpu_run(name, "step", elim))
    same_bits(chain, run_gpu(name, "chain", elim))


@pytest.mark.parametrize("name", bs.ATOMIC)
def test_atomic_schur_mode_matches_oracle(name):
    """(d) set_deterministic(False): the reduced system summed with FP64 atomics, the objects' update by k_obj_rows (a 6 x dimp row
    block in LDS, 2048 wide at b32) -- the same solver behind it, the same bars.  lambda only where chi2 still moves
    (test_vertices_without_edges_and_single_observation_landmarks: its update factor is a cubic in the relative gain)."""
    r = oracle_run(name)
    g = run_gpu(name, "chain", "elim", deterministic=False)
    moved = {}
    for key in ("2", "1"):
        c = np.asarray(r["t" + key]["chi2"], np.float64)
        moved[key] = np.concatenate([[True], (c[:-1] - c[1:]) > 1e-3 * c[:-1]])
    g = {k: (dict(v, lam=np.asarray(v["lam"])[moved[k[1]]]) if k[0] == "t" else v) for k, v in g.items()}
    r = {k: (dict(v, lam=np.asarray(v["lam"])[moved[k[1]]]) if k[0] == "t" else v) for k, v in r.items()}
    assert_matches_oracle("ba_blocks/%s/atomic/elim" % name, g, r)
