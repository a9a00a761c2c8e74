"""GPU: qsp_sim3_optimize_batch (Optimizer::OptimizeSim3 for all loop candidates in one launch) against tests/sim3_oracle.py.

Discrete outcomes (inlier flags, inlier counts, iteration and trial counts) must be exact; chi2 / lambda per iteration and the
refined Sim3 must lie within the bars of profiles/sim3_margins.json, which are 4 x the oracle's own sensitivity to the rounding
of its error evaluations (measured on the CPU, see that file).  A candidate's outputs must have the same bits alone, in any
batch and at any position."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import sim3_oracle as so

pytestmark = pytest.mark.gpu

BAR = json.load(open(so.MARGINS))["bar"]


def run(cands, fix_scale):
    from qsp_slam_amd.ba import optimize_sim3_batch
    return optimize_sim3_batch(cands, so.TH2, fix_scale, trace=True)


@pytest.fixture(scope="module")
def full():
    """the batch of 17, once per fix_scale setting"""
    return {fix: run(so.pool(fix), fix) for fix in (0, 1)}


@pytest.fixture(scope="module")
def wide():
    from qsp_slam_amd.ba import optimize_sim3_batch
    return optimize_sim3_batch(so.pool_wide(), so.TH2_WIDE, 1, trace=True)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("sim3", "inlier", "iters", "trace")) and a["n_inliers"] == b["n_inliers"]


@pytest.mark.parametrize("fix", [0, 1])
def test_batch_of_17_against_the_oracle(full, fix):
    worst = dict(chi2_rel=0.0, lambda_rel=0.0, sim3_abs=0.0)
    for i, (g, r) in enumerate(zip(full[fix], so.pool_results(fix))):
        assert np.array_equal(g["inlier"], r["inlier"]), i
        assert g["n_inliers"] == r["n_inliers"], i
        assert list(g["iters"]) == list(r["iters"]), (i, g["iters"], r["iters"])
        assert np.array_equal(g["trace"][:, :, 2], r["trace"][:, :, 2]), (i, g["trace"][:, :, 2], r["trace"][:, :, 2])
        d = so.sensitivity(g, r)
        print("fix_scale %d candidate %2d (%3d matches): %s" % (fix, i, len(r["inlier"]), d))
        worst = {k: max(worst[k], d[k]) for k in worst}
    print("fix_scale %d worst: %s  bars: %s" % (fix, worst, BAR))
    for k in worst:
        assert worst[k] <= BAR[k], (k, worst[k], BAR[k])


@pytest.mark.parametrize("fix", [0, 1])
def test_the_pools_cover_both_branches(full, fix):
    """the `< 10` rule (0 inliers, input returned, flags still reported), the 10- and the 5-iteration second call"""
    res, cands = full[fix], so.pool(fix)
    early = [i for i, (n, kind, _) in enumerate(so.POOL[fix]) if 0 < n < 10 or (n == 10 and kind == "outlier")]
    assert early and all(res[i]["n_inliers"] == 0 and np.array_equal(res[i]["sim3"], cands[i]["sim3"]) for i in early)
    assert any(res[i]["inlier"].sum() < len(res[i]["inlier"]) for i in early)
    assert res[0]["n_inliers"] == 0 and np.array_equal(res[0]["sim3"], cands[0]["sim3"]) and list(res[0]["iters"]) == [0, 0]
    assert any(r["n_inliers"] and r["n_inliers"] < len(r["inlier"]) for r in res)           # nBad > 0: optimize(10)
    if not fix:                                   # (fix_scale = 1: test_fixed_scale_clean_and_noisy_data_far_start_wide_gate)
        assert any(r["n_inliers"] and r["n_inliers"] == len(r["inlier"]) for r in res)      # nBad == 0: optimize(5)
    else:
        for r, c in zip(res, cands):
            assert r["sim3"][7] == c["sim3"][7]                                              # the scale comes back bit for bit


@pytest.mark.parametrize("fix", [0, 1])
def test_alone_in_any_batch_at_any_position(full, fix):
    cands = so.pool(fix)
    for i, c in enumerate(cands):                                                            # batches of 1
        assert same_bits(run([c], fix)[0], full[fix][i]), i
    three = run([cands[i] for i in so.BATCH3], fix)                                          # a batch of 3, other neighbours
    for r, i in zip(three, so.BATCH3):
        assert same_bits(r, full[fix][i]), i
    rev = run(cands[::-1], fix)                                                              # every other position
    for r, g in zip(rev[::-1], full[fix]):
        assert same_bits(r, g)
    again = run(cands, fix)                                                                  # and a repeated run
    assert all(same_bits(a, b) for a, b in zip(again, full[fix]))


def test_fixed_scale_clean_and_noisy_data_far_start_wide_gate(wide):
    """fix_scale = 1 on clean and noisy data (sim3_oracle.POOL_WIDE): Huber never active, no pair leaves, the second call is the
    5-iteration one; against the oracle as above, and alone as in the batch"""
    from qsp_slam_amd.ba import optimize_sim3_batch
    worst = dict(chi2_rel=0.0, lambda_rel=0.0, sim3_abs=0.0)
    for i, (g, r, c) in enumerate(zip(wide, so.pool_wide_results(), so.pool_wide())):
        n = len(c["info1"])
        assert g["inlier"].all() and g["n_inliers"] == n == r["n_inliers"], i
        assert list(g["iters"]) == list(r["iters"]) and 1 <= g["iters"][1] <= 5, (i, g["iters"], r["iters"])
        assert np.array_equal(g["trace"][:, :, 2], r["trace"][:, :, 2]), (i, g["trace"][:, :, 2], r["trace"][:, :, 2])
        assert g["sim3"][7] == c["sim3"][7]                                                  # the scale, bit for bit
        assert np.abs(g["sim3"] - c["true"]).max() < 1e-2 and np.abs(c["sim3"] - c["true"]).max() > 0.1
        d = so.sensitivity(g, r)
        print("wide candidate %d (%3d matches): %s" % (i, n, d))
        worst = {k: max(worst[k], d[k]) for k in worst}
        assert same_bits(optimize_sim3_batch([c], so.TH2_WIDE, 1, trace=True)[0], g), i
    print("wide worst: %s  bars: %s" % (worst, BAR))
    for k in worst:
        assert worst[k] <= BAR[k], (k, worst[k], BAR[k])


def test_single_form_of_the_python_wrapper():
    from qsp_slam_amd.ba import optimize_sim3, optimize_sim3_batch
    c = so.pool(0)[6]
    one = optimize_sim3(c, so.TH2, False)
    assert set(one) == {"sim3", "inlier", "n_inliers"} and one["inlier"].dtype == np.uint8 and one["sim3"].shape == (8,)
    r = so.pool_results(0)[6]
    assert one["n_inliers"] == r["n_inliers"] and np.array_equal(one["inlier"], r["inlier"])
    assert np.abs(one["sim3"] - r["sim3"]).max() <= BAR["sim3_abs"]
    assert optimize_sim3_batch([], so.TH2, False) == []


def test_error_paths_leave_the_outputs_untouched():
    from qsp_slam_amd import _lib
    L = _lib.lib()
    cands = [so.pool(0)[i] for i in (5, 2)]
    n = [len(c["info1"]) for c in cands]
    cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(c[k], np.float64) for c in cands]))
    K1, K2, S0 = (np.ascontiguousarray(np.stack([c[k] for c in cands])) for k in ("K1", "K2", "sim3"))
    arrs = [cat(k) for k in ("P1c", "P2c", "obs1", "obs2", "info1", "info2")]
    out, inl, ninl = np.full((2, 8), 7.0), np.full(sum(n), 9, np.uint8), np.full(2, -5, np.int32)
    tr = (_lib.Sim3Trace * 2)()
    tr[0].iters[0] = 77

    def call(off, drop=None, n_cand=2):
        p = [_lib.dptr(K1), _lib.dptr(K2), _lib.dptr(S0)] + [_lib.dptr(a) for a in arrs]
        outs = [_lib.dptr(out), _lib.u8ptr(inl), _lib.i32ptr(ninl)]
        o = _lib.i32ptr(np.asarray(off, np.int32))
        if drop == "off":
            o = None
        elif drop is not None and drop < 9:
            p[drop] = None
        elif drop is not None:
            outs[drop - 9] = None
        return L.qsp_sim3_optimize_batch(0, n_cand, o, *p, so.TH2, 0, *outs, tr)

    untouched = lambda: (out == 7.0).all() and (inl == 9).all() and (ninl == -5).all() and tr[0].iters[0] == 77
    for off in ([0, n[0], n[0] - 1], [0, -3, n[0]], [-1, n[0], n[0] + n[1]], [1, n[0], n[0] + n[1]]):
        assert call(off) == _lib.QSP_ERR_INVALID and untouched(), off
    good = [0, n[0], n[0] + n[1]]
    for drop in ["off"] + list(range(12)):
        assert call(good, drop) == _lib.QSP_ERR_INVALID and untouched(), drop
    assert call(good, n_cand=-1) == _lib.QSP_ERR_INVALID and untouched()
    assert call(good, n_cand=0) == _lib.QSP_OK and untouched()
    assert L.qsp_sim3_optimize_batch(0, 0, *([None] * 10), so.TH2, 0, None, None, None, None) == _lib.QSP_OK
    assert call(good) == _lib.QSP_OK and not untouched()
    assert list(ninl) == [so.pool_results(0)[5]["n_inliers"], so.pool_results(0)[2]["n_inliers"]]
