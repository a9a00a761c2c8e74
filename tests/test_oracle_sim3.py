"""CPU: tests/sim3_oracle.py, the float64 restatement of Optimizer::OptimizeSim3 that qsp_sim3_optimize_batch is held to, checked
on its own -- and the conditions the GPU fixtures must meet as INPUTS (same decisions whether the edge errors are evaluated in
float64 or in longdouble, no final chi2 near th2), asserted here where no GPU is involved."""
import json

import numpy as np
import pytest

from tests import sim3_oracle as so


def test_numeric_jacobian_agrees_with_the_analytic_one():
    """A float64 error of a few hundred pixels carries ~1e-13 of rounding, which the factor 5e8 turns into ~1e-4 on Jacobian
    entries of 1e2..1e4: 1e-5 of the largest entry per match is the bound; observed 2e-8..2e-7."""
    worst = 0.0
    for fix in (0, 1):
        for c in so.pool(fix):
            if not len(c["info1"]):
                continue
            Jn, Ja = so.numeric_jacobian(c["sim3"], c, fix), so.analytic_jacobian(c["sim3"], c)
            if fix:
                assert not Jn[:, :, 6].any()                       # update[6] = 0 inside the oplus: the column is exactly zero
                Ja[:, :, 6] = 0
            worst = max(worst, float(np.max(np.abs(Jn - Ja).max(axis=(1, 2)) / np.abs(Ja).max(axis=(1, 2)))))
    print("numeric against analytic Jacobian, worst relative difference: %.2e" % worst)
    assert worst < 1e-5


@pytest.mark.parametrize("fix", [0, 1])
def test_exact_data_stays_put_and_keeps_every_pair(fix):
    c = so.make_candidate(5, 40, "exact", fix)
    c["obs1"], c["obs2"] = (so.errors(c["true"], dict(c, obs1=0 * c["obs1"], obs2=0 * c["obs2"]))[i] * -1 for i in (0, 1))
    r = so.optimize_sim3(c, so.TH2, fix)
    assert r["n_inliers"] == 40 and r["inlier"].all()
    assert np.abs(r["sim3"] - c["true"]).max() < 1e-9


@pytest.mark.parametrize("fix", [0, 1])
def test_a_perturbed_start_recovers_the_known_sim3(fix):
    c = so.make_candidate(3, 80, "clean", fix)                     # 0.05 px of noise
    assert np.abs(c["sim3"] - c["true"]).max() > 1e-2
    r = so.optimize_sim3(c, so.TH2, fix)
    assert r["n_inliers"] == 80
    assert np.abs(r["sim3"] - c["true"]).max() < 1e-3
    if fix:
        assert r["sim3"][7] == c["sim3"][7]                        # bit for bit
    else:
        assert r["sim3"][7] != c["sim3"][7]


def test_outliers_take_the_10_iteration_branch_clean_data_the_5_iteration_one():
    res = so.pool_results(0)
    seen = set()
    for i, (n, kind, _) in enumerate(so.POOL[0]):
        if n < 10 or res[i]["n_inliers"] == 0:
            continue
        if kind == "outlier":
            assert int(res[i]["inlier"].sum()) < n and res[i]["n_more"] == 10
        else:
            assert res[i]["n_inliers"] == n and res[i]["n_more"] == 5 and res[i]["iters"][1] <= 5
        seen.add(res[i]["n_more"])
    assert seen == {5, 10}


def test_fixed_scale_clean_and_noisy_data_take_the_5_iteration_branch():
    for r, c, (n, kind, _) in zip(so.pool_wide_results(), so.pool_wide(), so.POOL_WIDE):
        assert r["n_inliers"] == n and r["inlier"].all() and r["n_more"] == 5 and 1 <= r["iters"][1] <= 5
        assert r["sim3"][7] == c["sim3"][7] and np.abs(r["sim3"] - c["true"]).max() < 1e-2
        assert r["final_chi2"].max() < float(np.float32(so.TH2_WIDE))          # Huber's zone starts at th2: never entered at the end
    assert {k for _, k, _ in so.POOL_WIDE} == {"clean", "noisy"}


def test_fewer_than_10_pairs_left_returns_0_and_the_input():
    for fix in (0, 1):
        for i, (n, kind, _) in enumerate(so.POOL[fix]):
            r, c = so.pool_results(fix)[i], so.pool(fix)[i]
            if n < 10 or (n == 10 and kind == "outlier"):
                assert r["n_inliers"] == 0 and np.array_equal(r["sim3"], c["sim3"]) and r["iters"][1] == 0
                if kind == "outlier":
                    assert not r["inlier"].all()                   # the bad flags are still reported


@pytest.mark.parametrize("fix", [0, 1])
def test_fixture_conditions(fix):
    for i, (a, b) in enumerate(zip(so.pool_results(fix, False), so.pool_results(fix, True))):
        assert so.same_decisions(a, b), (fix, i)
        assert so.chi2_clear_of_threshold(a) and so.chi2_clear_of_threshold(b), (fix, i)
    for p in so.POOL.values():                                      # no candidate twice (index parity = camera order)
        assert len({(e, i & 1) for i, e in enumerate(p)}) == len(p)


def test_fixture_conditions_of_the_wide_gate_pool():
    for i, (a, b) in enumerate(zip(so.pool_wide_results(False), so.pool_wide_results(True))):
        assert so.same_decisions(a, b), i
        assert so.chi2_clear_of_threshold(a, so.TH2_WIDE) and so.chi2_clear_of_threshold(b, so.TH2_WIDE), i


def test_committed_bars_are_4x_the_measured_sensitivity():
    doc = json.load(open(so.MARGINS))
    sens = so.measured_sensitivity()
    print("sensitivity now: %s  committed: %s" % (sens, doc["sensitivity"]))
    for k, v in doc["sensitivity"].items():
        assert doc["bar"][k] == 4 * v
        assert sens[k] <= doc["bar"][k]                            # (libm may move the float64 run a little between hosts)
