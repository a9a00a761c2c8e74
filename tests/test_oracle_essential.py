"""CPU: tests/essential_oracle.py, the oracle of qsp_essential_graph_optimize, against closed-form facts; and the conditions its
fixtures must meet for the GPU comparison to be meaningful, checked by the oracle alone."""
import numpy as np
import pytest

from tests import essential_oracle as eo
from tests.sim3_oracle import s_exp, s_inv, s_mul


@pytest.mark.parametrize("u", [
    [0.3, 0.2, -0.1, 1.0, 2.0, 3.0, 0.2],            # neither small
    [1e-7, 2e-7, 0.0, 1.0, 2.0, 3.0, 0.2],           # small angle
    [0.3, 0.2, -0.1, 1.0, 2.0, 3.0, 1e-7],           # small sigma
    [1e-7, 0.0, 1e-7, 1.0, 2.0, 3.0, 1e-8],          # both small
])
def test_log_inverts_exp_on_all_four_branches(u):
    u = np.array(u)
    assert np.abs(eo.s_log(s_exp(u)) - u).max() < 1e-12


def test_numeric_jacobian_agrees_with_a_wide_step_longdouble_one():
    """the 1e-9 quotient's noise: the translations inside an error evaluation reach ~20 here (ring of radius 6, two products), so
    each of its ~10 roundings is up to 20 x 2^-53 = 2.2e-15; two evaluations, times 5e8, times |W^-1| <= 3 in Sim3::log's
    upsilon = W^-1 t: 1.3e-4 absolute at worst, on entries of size 1 and more"""
    sc = eo.fixture("free10")
    S = sc["sim3"]
    slot = np.where(sc["fixed"] == 0, 0, -1)
    g = dict(v0=sc["v0"].astype(np.int64), v1=sc["v1"].astype(np.int64), meas=sc["meas"], fixed=sc["fixed"], fix_scale=False, slot=slot)
    Jn, Ja = eo.numeric_jacobian(S, g), eo.analytic_jacobian(S, g)
    free = np.stack([sc["fixed"][g["v0"]] == 0, sc["fixed"][g["v1"]] == 0], -1)
    err = np.abs(Jn - Ja)[free]
    assert free.any() and not free.all()
    assert err.max() < 1.3e-4 and np.abs(Ja[free]).max() > 0.5, err.max()
    g["fix_scale"] = True
    assert np.all(eo.numeric_jacobian(S, g)[:, :, 6, :] == 0.0)               # the scale column is exactly 0


@pytest.mark.parametrize("fix_scale", [False, True])
def test_consistent_graph_stays_and_one_bad_loop_edge_is_reduced(fix_scale):
    sc = eo.make_scene(3, 9, fixed_at=4, fix_scale=fix_scale, n_pt=5, n_iter=3, consistent=True)
    assert eo.chi2(sc) < 1e-25
    r = eo.optimize(sc)
    assert np.abs(r["sim3"] - sc["sim3"]).max() < 1e-9 and r["trace"][-1, 0] < 1e-25
    assert np.array_equal(r["sim3"][4], sc["sim3"][4])
    bad = dict(sc)
    bad["meas"] = sc["meas"].copy()
    k = 0                                                                      # the loop edge
    bad["meas"][k] = s_mul(s_exp(np.array([0.02, -0.01, 0.03, 0.1, -0.05, 0.08, 0.0 if fix_scale else 0.03])), sc["meas"][k])
    c0 = eo.chi2(bad)
    r = eo.optimize(bad)
    assert c0 > 1e-3 and r["trace"][-1, 0] < 0.75 * c0
    assert np.array_equal(r["sim3"][4], sc["sim3"][4])                         # the fixed vertex keeps its bits
    assert np.abs(r["sim3"] - sc["sim3"]).max() > 1e-3


def test_point_whose_reference_is_the_fixed_vertex_stays():
    sc = eo.fixture("free10")
    r = eo.fixture_result("free10")
    at_fixed = np.flatnonzero(sc["ref"] == 5)
    assert len(at_fixed) and np.abs(r["pts"][at_fixed] - sc["pts"][at_fixed]).max() < 1e-14
    assert np.abs(r["pts"] - sc["pts"]).max() > 1e-3
    S = sc["sim3"][5]
    assert np.abs(s_mul(s_inv(S), S) - np.array([0, 0, 0, 0, 0, 0, 1, 1.0])).max() < 1e-15


@pytest.mark.parametrize("name", list(eo.FIXTURES))
def test_fixture_decisions_do_not_depend_on_rounding(name):
    a, b, c = eo.fixture_result(name), eo.fixture_result(name, True, False), eo.fixture_result(name, False, True)
    assert eo.same_decisions(a, b), (a["accepts"], b["accepts"])
    assert eo.same_decisions(a, c), (a["accepts"], c["accepts"])
    assert a["margin"] >= eo.MIN_MARGIN, a["margin"]
    assert a["iters"] <= eo.TRACE_MAX
    if name.startswith("stop"):
        assert a["stopped_by_rule"] and a["iters"] < eo.FIXTURES[name]["n_iter"]
    else:
        assert a["iters"] == eo.FIXTURES[name]["n_iter"]


def test_the_fixtures_cover_the_cases():
    sc = {k: eo.fixture(k) for k in eo.FIXTURES}
    n_free = {k: int((v["fixed"] == 0).sum()) for k, v in sc.items()}
    assert {n_free[k] for k in ("free1", "free9", "free10", "free19", "free19_tight")} == {1, 9, 10, 19} and n_free["kf40"] == 39
    where = {int(np.flatnonzero(v["fixed"])[0]) * 2 // max(len(v["fixed"]) - 1, 1) for v in sc.values()}
    assert where == {0, 1, 2}                                                  # first, middle, last
    hub = sc["hub"]
    assert max(np.bincount(np.concatenate([hub["v0"], hub["v1"]]))) > 64 and len(hub["v0"]) > 64
    for d in (sc["free19"], sc["free19_tight"]):
        pairs = list(zip(d["v0"], d["v1"]))
        assert len(pairs) - len(set(pairs)) >= 5
    assert eo.bars("free19_tight")["sim3_abs"] < 1e-4
    d = sc["free19"]
    pairs = list(zip(d["v0"], d["v1"]))
    assert len(pairs) - len(set(pairs)) >= 5
    for v in sc.values():                                                      # the fixed vertex as v0 and as v1
        f = int(np.flatnonzero(v["fixed"])[0])
        assert (v["v1"] == f).any()
    assert any((v["v0"] == int(np.flatnonzero(v["fixed"])[0])).any() for v in sc.values())
    assert {len(v["pts"]) for v in sc.values()} >= {0, 1, 130}
    assert any(any(len(t) > 1 for t in eo.fixture_result(k)["accepts"]) for k in sc)      # rejected trials occur
    s = eo.measured_sensitivity()
    assert set(s) == set(eo.FIXTURES) and all(0 < v["sim3_abs"] < 2e-2 and 0 < v["chi2_rel"] < 2e-3 for v in s.values()), s
