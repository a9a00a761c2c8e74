"""CPU: the cases of tests/test_gpu_ray_edges.py (tests/ray_edges.py) meet the conditions their seeds were chosen for, on the oracle
alone -- no threshold decision of the float32 iteration within reach of rounding, the float32 and the float64 oracle with the same
lists and, in every small group of rows, the same rows to half the bar, every ray pass and depth stage observed by a kept row --
the exit scenes end in the exits they are named after, and the comparisons of the GPU test can fail: a stale depth table and a
depth step of (d_max - d_min) / D end ten bars and more away."""
import numpy as np
import pytest

from oracle import sdf_oracle as so
from tests import ray_edges as re_


@pytest.mark.parametrize("name", list(re_.CASES))
def test_case_meets_the_conditions_its_seed_was_chosen_for(name):
    case = re_.build_case(name)
    n_fg, n_bg, D, _ = re_.CASES[name]
    it, it64 = case["it"], case["it64"]
    assert it["fail"] is None and it64["fail"] is None and case["cfg"].n_depth == D
    assert case["obj"]["rays"].shape == (n_fg + n_bg, 3) and case["obj"]["pts"].shape == (re_.M_PTS, 3)
    assert it["H"].dtype == np.float32 and it64["H"].dtype == np.float64
    fig = re_.conditions(case)
    print("ray_edges/%s: %s" % (name, fig))
    assert fig["ball"] >= re_.BALL_MARGIN and fig["band"] >= re_.BAND_MARGIN and fig["keep"] >= re_.KEEP_MARGIN          # 1, 2, 3
    assert fig["same_lists"]                                                                                             # 4
    assert fig["small_group_rows"] <= 0.5 * re_.ROW_TOL                                                                   # 5
    assert fig["rays_without_sample"] >= 1 and fig["n_valid"] >= 10 and fig["K"] >= 1                                   # 6
    if name in re_.RAY_CASES:
        n_pass = (n_fg + n_bg + re_.SCAN_RAYS - 1) // re_.SCAN_RAYS
        assert len(fig["rows_per_group"]) == n_pass and min(fig["rows_per_group"]) >= 1
        if (n_fg + n_bg) % re_.SCAN_RAYS == 1:                        # 513, 1025 (and 1537): the last pass is one ray
            assert fig["last_ray_kept"]
    else:
        assert (n_fg, n_bg) == (200, 100)
        assert fig["K"] >= 2 or D < 4
        assert fig["top_k"] <= D - 2                                  # k = 0 and k = D - 1 lie on the unit sphere: never inside
        if D == 64:
            assert fig["top_k"] == 62
        if D == 3:
            assert set(case["rt"]["valid_k"]) == {1}
    assert re_.conditions_hold(case, fig)
    assert so.F32 is np.float32 and so.render_term.__name__ == "render_term"        # the oracle is as it was


def test_the_case_table_is_the_one_the_kernels_need():
    assert [re_.CASES[n][:2] for n in re_.RAY_CASES] == [(511, 0), (512, 0), (513, 0), (1024, 0), (1025, 0), (1100, 437)]
    assert all(re_.CASES[n][2] == 50 for n in re_.RAY_CASES)
    assert [re_.CASES[n][2] for n in re_.DEPTH_CASES] == [3, 4, 5, 7, 49, 63, 64]
    assert set(re_.STAGED) == {"r513", "r1100+437", "d3", "d4", "d5", "d63", "d64"}
    # four k_scan passes, two k_sample passes, seven k_stage_list passes
    n = sum(re_.CASES["r1100+437"][:2])
    assert (-(-n // 512), -(-n // 1024), -(-n // 256)) == (4, 2, 7)


def test_the_exit_scenes_end_in_their_exits():
    n_fg, n_bg, D, seed = re_.NONE_CASE
    c = re_.build(n_fg, n_bg, D, seed)
    assert D == 2 and c["it"]["fail"] == "render_none" and c["it64"]["fail"] == "render_none" and c["rt"] is None
    assert re_.margins_hold(re_.decision_margins(c))                  # (fewer than 10 valid samples on the GPU too)
    n_fg, n_bg, D, seed, n_pts = re_.NAN_CASE
    c = re_.build(n_fg, n_bg, D, seed, n_pts)
    fig = re_.decision_margins(c)
    print("ray_edges/render_nan: n_valid %d %s" % (c["it"]["n_valid"], fig))
    for it in (c["it"], c["it64"]):
        assert it["fail"] == "render_nan" and it["n_valid"] >= 10 and it["K"] == 0
    assert c["it"]["n_valid"] == c["it64"]["n_valid"] == c["rt"]["n_valid"] and c["rt"]["res"].shape == (0,)
    assert re_.margins_hold(fig)
    # no rays at all: the reference's `< 10 valid samples` exit
    o = re_.no_ray_object()
    assert o["rays"].shape == (0, 3) and [x["rays"].shape[0] for x in re_.ragged_objects()] == [0, 40, 513, 1025]
    it = so.gn_iteration(re_.oracle_decoder(), so.JointConfig(), c["T_oc"], np.zeros(64, np.float32), o["pts"], o["rays"], o["depth"], 0)
    assert it["fail"] == "render_none"
    r = so.reconstruct_object(re_.oracle_decoder(), so.JointConfig(), o["t_cam_obj"], o["pts"], o["rays"], o["depth"])
    assert r["is_good"] is False and r["t_cam_obj"] is None and r["loss"] == 0.0


def test_a_stale_depth_table_ends_ten_bars_away():
    """render rows computed with the observed depth of ray r - 512 for the rays r >= 512 (a row table of k_scan that was not
    refilled, or an index that forgot its pass): column 71 ends at least ten bars from the oracle's"""
    case = re_.build_case("r1100+437")
    c, rt, cfg = case["call"], case["rt"], case["cfg"]
    stale = c["depth_obs"].copy()
    stale[re_.SCAN_RAYS:] = c["depth_obs"][:-re_.SCAN_RAYS]
    d_u = c["depth_obs"][rt["ray"]] - rt["res"]                       # rendered depth of the rows whose residual is not clamped
    free = np.abs(rt["res"]) < np.float32(0.30)
    res_stale = np.clip(stale[rt["ray"]] - d_u, np.float32(-0.30), np.float32(0.30)).astype(np.float32)
    good, bad = so.robust_residual(rt["res"], cfg.b1)[0], so.robust_residual(res_stale, cfg.b1)[0]
    assert np.array_equal(good[rt["ray"] < re_.SCAN_RAYS], bad[rt["ray"] < re_.SCAN_RAYS])       # (the first pass is untouched)
    err = np.abs(bad - good)[free] / np.abs(good).max()
    groups = (rt["ray"] // re_.SCAN_RAYS)[free]
    print("ray_edges/stale_table: column 71 off by %s bars per pass" % [float(err[groups == g].max() / re_.RES_TOL) for g in range(1, 4)])
    for g in range(1, 4):
        assert err[groups == g].max() >= 10 * re_.RES_TOL, g


@pytest.mark.parametrize("name", ["d3", "d4", "d5"])
def test_a_depth_step_over_D_ends_ten_bars_away(name):
    """delta_d = (d_max - d_min) / D in place of / (D - 1): every Jacobian row of the render term is off by 1 / D of itself"""
    case = re_.build_case(name)
    it, D = case["it"], case["D"]
    wrong = np.float32((D - 1) / D)
    err = re_.jacobian_row_errors(it["Jp_render"] * wrong, it["Jc_render"] * wrong, it)
    groups, n_groups = re_.row_groups(case)
    ok, worst, _ = re_.grouped_rows_ok(err, groups, n_groups)
    print("ray_edges/%s/step_over_D: rows off by %.0f bars" % (name, worst / re_.ROW_TOL))
    assert not ok and worst >= 10 * re_.ROW_TOL
    same = re_.jacobian_row_errors(it["Jp_render"], it["Jc_render"], it)
    assert re_.grouped_rows_ok(same, groups, n_groups)[0]
