"""CPU: the stage oracle of qsp_essential_graph_stages (essential_oracle.linearise / trial over STAGE_SCENES) and the conditions
its scenes must meet for tests/test_gpu_essential_stages.py to reach the code paths it is about, checked by the oracle alone.  The
reference distances measured here are the GPU test's bars (essential_oracle.stage_bars; profiles/essential_stage_margins.json
records them, python -m tests.essential_oracle)."""
import json

import numpy as np
import pytest

from tests import essential_oracle as eo
from tests.sim3_oracle import s_exp

NAMES = list(eo.STAGE_SCENES)


def dims(name):
    g = eo.graph_of(eo.stage_scene(name))
    return g["D"] * g["n_free"]


def test_the_scenes_have_the_sizes_the_table_names():
    assert {n: dims(n) for n in NAMES} == dict(kf2=7, kf2_fs=6, kf10=63, kf11=70, kf33_fs=192, kf65=448, hub4=140, hub4_fs=120,
                                                kf40_4fs=216, isolated=84, branches=56)
    for name, dim in eo.EXACT_BLOCKS.items():
        assert dims(name) == dim and dim % 64 == 0
    assert all(dims(n) % 64 for n in NAMES if n not in eo.EXACT_BLOCKS)        # every other scene has the identity tail
    assert (dims("kf40_4fs") + 63) // 64 == 4 and (dims("kf65") + 63) // 64 == 7


@pytest.mark.parametrize("name", eo.MULTI_FIXED)
def test_multi_fixed_scenes_reach_the_paths(name):
    sc = eo.stage_scene(name)
    g = eo.graph_of(sc)
    fx = g["fixed"].astype(bool)
    assert fx.sum() == 4 and fx[g["v0"]].any() and fx[g["v1"]].any()
    assert (fx[g["v0"]] & fx[g["v1"]]).any()                                   # an edge with both ends fixed
    v = np.flatnonzero(~fx)
    assert ((g["slot"][v] != v) & (g["slot"][v] != v - 1)).any()               # a slot that is neither v nor v - 1
    if name.startswith("hub4"):
        assert fx[3] and fx[23] and not fx[9]
        assert (g["v0"] == 9).sum() + (g["v1"] == 9).sum() > 64                # the hub is free, more than 64 incident edges,
        assert (g["v0"] == 9).sum() > 3 and (g["v1"] == 9).sum() > 3           # in both orientations
        pairs = list(zip(g["v0"], g["v1"]))
        assert len(pairs) > 128 and len(pairs) - len(set(pairs)) >= 5


def test_the_isolated_vertex_has_no_edge_and_a_zero_block():
    sc = eo.stage_scene("isolated")
    g = eo.graph_of(sc)
    v = len(sc["sim3"]) - 1
    assert not g["fixed"][v] and not (g["v0"] == v).any() and not (g["v1"] == v).any()
    E, chi, J, H, b = eo.linearise(sc, sc["sim3"])
    i = slice(7 * g["slot"][v], 7 * g["slot"][v] + 7)
    assert not H[i].any() and not H[:, i].any() and not b[i].any()
    for lam in eo.stage_lambdas(H):
        x, St, _, _ = eo.trial(sc, sc["sim3"], H, b, lam)
        assert not x[i].any() and np.abs(St[v] - sc["sim3"][v]).max() < 1e-15


def test_branches_takes_each_branch_of_the_logarithm_twice():
    sc = eo.stage_scene("branches")
    g = eo.graph_of(sc)
    S = sc["sim3"]
    Er = eo.mul_b(eo.mul_b(g["meas"], S[g["v0"]]), eo.inv_b(S[g["v1"]]))
    small_s, small_a = eo.log_branches(Er)
    for s in (False, True):
        for a in (False, True):
            assert ((small_s == s) & (small_a == a)).sum() == 2, (s, a)
    E = eo.edge_errors(g["meas"], S[g["v0"]], S[g["v1"]])
    theta = np.linalg.norm(E[:, :3], axis=1)
    assert theta.max() < 2.5 and not ((theta > 1e-3) & (theta < 2e-2)).any()  # away from the threshold, theta ~ 4.5e-3
    assert np.abs(theta - np.tile(eo.BRANCH_ROT, 2)).max() < 1e-8 and np.abs(E[:, 6] - np.repeat(eo.BRANCH_SIGMA, 4)).max() < 1e-12


def test_no_scene_comes_near_a_branch_threshold_or_pi():
    for name in NAMES:
        sc = eo.stage_scene(name)
        g = eo.graph_of(sc)
        E = eo.edge_errors(g["meas"], sc["sim3"][g["v0"]], sc["sim3"][g["v1"]])
        theta = np.linalg.norm(E[:, :3], axis=1)
        assert theta.max() < 2.5 and not ((theta > 3e-3) & (theta < 7e-3)).any(), name
        if name != "branches":                                                 # (its sigma is exactly 0 or 0.1 by construction)
            assert np.abs(E[:, 6]).max() < 1e-12 if sc["fix_scale"] else np.abs(E[:, 6]).min() > 1e-4, name


@pytest.mark.parametrize("u", [[0.3, 0.2, -0.1, 1.0, 2.0, 3.0, 0.2], [1e-7, 2e-7, 0.0, 1.0, 2.0, 3.0, 0.2], [0.3, 0.2, -0.1, 1.0, 2.0, 3.0, 1e-7],
                               [1e-7, 0.0, 1e-7, 1.0, 2.0, 3.0, 1e-8], [2.0, -1.5, 1.0, 0.1, 0.2, 0.3, -0.4], [0, 0, 0, 0, 0, 0, 0]])
def test_the_longdouble_exponential_is_the_float64_one(u):
    assert np.abs(eo.exp_ld(u).astype(np.float64) - s_exp(np.array(u, np.float64))).max() < 2e-15


@pytest.mark.parametrize("name", ["kf40_4fs", "hub4", "hub4_fs", "kf11"])
def test_the_assembled_matrix_is_symmetric_in_every_bit(name):
    sc = eo.stage_scene(name)
    E, chi, J, H, b = eo.linearise(sc, sc["sim3"])
    assert np.array_equal(H, H.T) and np.abs(H).max() > 1


def test_fixed_sides_and_the_fixed_scale_column_are_zero():
    for name in ("hub4", "hub4_fs"):
        sc = eo.stage_scene(name)
        g = eo.graph_of(sc)
        J = eo.numeric_jacobian(sc["sim3"], g)
        fx = g["fixed"].astype(bool)
        assert not J[fx[g["v0"]], 0].any() and not J[fx[g["v1"]], 1].any() and J[~fx[g["v0"]], 0].any()
        if sc["fix_scale"]:
            assert not J[:, :, 6, :].any()


def test_trial_takes_x_from_outside_and_the_blocked_solve_is_a_solve():
    sc = eo.stage_scene("kf11")
    E, chi, J, H, b = eo.linearise(sc, sc["sim3"])
    lam = eo.stage_lambdas(H)[1]
    x, St, c2, scale = eo.trial(sc, sc["sim3"], H, b, lam)
    x2, St2, c22, scale2 = eo.trial(sc, sc["sim3"], H, b, lam, x=x.copy())
    assert np.array_equal(x, x2) and np.array_equal(St, St2) and c2 == c22 and scale == scale2
    assert c2 < eo.chi2_lanes(chi) and scale > 0                                # the step reduces chi2
    assert np.abs(eo.solve_blocked(H, b, lam) - x).max() < 1e-12 * np.abs(x).max()
    f = int(np.flatnonzero(sc["fixed"])[0])
    assert np.array_equal(St[f], sc["sim3"][f])


@pytest.mark.parametrize("name", NAMES)
def test_reference_distances(name):
    """the oracle's own distances stage by stage: everything but the difference quotient is rounding, the quotient's noise is the
    5e8-fold rounding of an error evaluation (~5e-6 on entries up to ~12), and float64 numeric lies ~4e-6 from the wide-step
    longdouble derivative.  On `branches` the latter says nothing: the edges with sigma exactly 0 sit on the small-sigma branch, the
    wide step (1e-5, 2e-5) leaves it, and the other branch's B = (sigma^2 / 2 - sigma + 1) s / sigma^3 (g2o's formula as it stands)
    is not the limit of the first."""
    s = eo.stage_sensitivity(name)
    print(name, json.dumps(s))
    assert 0 < s["E_abs"] < 1e-14 and 0 < s["update_abs"] < 1e-13 and 0 < s["pt_abs"] < 1e-14
    assert 1e-7 < s["J_abs"] < 1e-5
    if name != "branches":
        assert 1e-7 < s["J_analytic_abs"] < 1e-5
    assert len(s["lambdas"]) == 3 and s["lambdas"][0] == 1e-16 and s["lambdas"][2] == 30.0 and 1e-16 < s["lambdas"][1] < 30
    assert all(0 < v < 1e-12 for v in s["x_rel"] + s["x_blocked_rel"])
    bar = eo.stage_bars(name)
    assert bar["E_abs"] == eo.FACTOR * s["E_abs"] and bar["x_rel"] == [eo.FACTOR * v for v in s["x_rel"]]


def test_the_margins_file_lists_every_scene():
    doc = json.load(open(eo.STAGE_MARGINS))
    for part in ("sensitivity", "bar"):
        assert set(doc[part]) == set(NAMES)
        assert all(set(eo.stage_bars(n)) <= set(doc[part][n]) for n in NAMES)
    assert set(doc["fixture_pt_bar"]) == set(eo.FIXTURES)
