"""The conditions under which tests/test_gpu_pose_only.py decides something, checked on the oracle alone (no GPU):

* the inlier filter behind iteration index 4 is nowhere on a knife edge: every residual of that iteration, in every case, is at
  least 1e-3 away from the filter's 0.05 -- the decoder pipes agree with float64 to about 1e-5 on a value, so the library's mask
  must be the oracle's, with no point left out of the comparison; the filter removes points in the filter cases, all of them in the
  emptied object, and none anywhere else;
* the step comparison bites: at iterations 0 and 5 the oracle's step recomputed with the last point left out, with the last point
  counted twice, and (behind the filter) with the divisor left at the uploaded count is more than 10 bars away from the true step.
  One entry cannot meet this and is recorded, not asserted: the one-point case at iteration 5.  A single point is one equation in
  six unknowns; Gauss-Newton contracts its residual by about 1e-2 / |J|^2 per iteration wherever it starts, so by iteration 5 the
  step is 1e-5 of a unit and below, where its own float32 rounding (the yardstick) is of order 1e-2 .. 1e-1 of it -- and a start far
  enough out to converge slowly has |res| > 0.05 at iteration 4, which the filter then removes.  With the point left out the step
  is the identity, 30 bars away; counted twice it moves by half a percent, which that bar cannot see (0.17 bars; more than 0.1
  is asserted).  No GPU test relies on it:
  iteration 5 is compared on the filter cases, and the one-point case is compared at iterations 0 .. 4;
* the yardstick: per case and iteration the float32 oracle's distance from its own float64 evaluation of the same iteration, from
  which the GPU tests' bar max(4 x yardstick, 1e-4) follows (recorded through tests/margins.py: profiles/pose_only_margins.json).
"""
import numpy as np
import pytest

from oracle import sdf_oracle as so
from tests import pose_only_cases as pc
from tests.margins import within

GUARD_BARS = 10.0
NOT_ACHIEVABLE = {("m1", 5, "last_point_twice")}      # (see the module docstring)
NOT_ACHIEVABLE_FLOOR = 0.1                            # what does hold there (0.17 bars): held, so that the entry cannot drift silently


@pytest.mark.parametrize("name", pc.ALL)
def test_the_filter_is_nowhere_on_a_knife_edge_and_removes_what_the_case_says(name):
    r = pc.run(name)
    res = r["trace"][4]["res"]
    m = r["case"]["pts"].shape[0]
    assert res.shape == (m,) and r["trace"][4]["n"] == m                  # every point is compared: the share left out is 0
    edge = float(np.abs(np.abs(res.astype(np.float64)) - so.POSE_ONLY_INLIER).min())
    kept = r["kept"]
    print("pose_only/%s: %d points, %d kept, nearest |res| to 0.05 at iteration 4: %.3g" % (name, m, int(kept.sum()), edge))
    assert edge >= pc.KNIFE_EDGE
    assert np.array_equal(kept, np.abs(res) <= 0.05)
    if name in pc.FILTER:
        assert 0 < kept.sum() < m and r["trace"][5]["n"] == kept.sum() and (~kept[::7]).sum() >= m // 14      # mostly the planted ones
    elif name == pc.EMPTIED:
        assert not kept.any()
    else:
        assert kept.all() and r["trace"][5]["n"] == m


def test_the_oracle_returns_a_non_finite_pose_for_the_emptied_object():
    c = pc.case(pc.EMPTIED)
    with np.errstate(all="ignore"):
        try:
            out = so.estimate_pose_cam_obj(pc.oracle_decoder("big"), so.JointConfig(n_iter_pose=6), c["t_co_se3"], c["scale"], c["pts"],
                                           c["code"])
        except np.linalg.LinAlgError:      # (a LAPACK that reports the NaN matrix as singular: no pose at all)
            return
    assert not np.isfinite(out).all()
    assert np.isfinite(pc.oracle_pose(pc.EMPTIED, 5)).all()           # ... while five iterations, which never filter, give one


def test_the_trace_is_additive_and_the_result_unchanged():
    """the records' new entries change nothing of what estimate_pose_cam_obj returned before: the state after each iteration is
    exp(dx) T_oc in float32, the result the inverse of the last state with the scale taken out"""
    c = pc.case("filter_m65")
    dec = pc.oracle_decoder("big")
    for n_iter in (5, 6, 8):
        out = so.estimate_pose_cam_obj(dec, so.JointConfig(n_iter_pose=n_iter), c["t_co_se3"], c["scale"], c["pts"], c["code"])
        assert np.array_equal(out, pc.oracle_pose("filter_m65", n_iter))
    for it in pc.run("filter_m65")["trace"]:
        assert set(it) >= {"T_oc", "H", "b", "dx", "n", "res", "T_oc_new", "f64"} and it["res"].shape == (it["n"],)
        assert it["H"].dtype == np.float32 and it["f64"]["H"].dtype == np.float64
        assert np.array_equal(it["T_oc_new"], (so.exp_se3(it["dx"]) @ it["T_oc"]).astype(np.float32))


@pytest.mark.parametrize("name", pc.ALL)
def test_yardstick_of_every_step(name):
    """the float32 oracle against its float64 flavour, per iteration; a step that meets its own bar by construction (x 4)"""
    r = pc.run(name)
    for e in range(r["n_done"]):
        y, bar = pc.yardstick(name, e), pc.bar(name, e)
        size = float(np.abs(pc.oracle_step(name, e) - np.eye(4)).max())
        print("pose_only/%s/it%d: |step - I| %.3g  yardstick %.3g  bar %.3g" % (name, e, size, y, bar))
        assert np.isfinite(y) and within("pose_only/%s/it%d/yardstick_f32_vs_f64" % (name, e), y, bar)
        f32, f64 = r["trace"][e], r["trace"][e]["f64"]
        assert f64["n"] == f32["n"] and np.abs(f64["res"] - f32["res"]).max() < 1e-5


@pytest.mark.parametrize("name", pc.SINGLE + pc.FILTER)
def test_a_defective_step_is_more_than_10_bars_away(name):
    for e in (0, 5):
        true, bar = pc.oracle_step(name, e), pc.bar(name, e)
        defects = pc.defect_steps(name, e)
        assert ("divisor_at_uploaded_count" in defects) == (e == 5 and name in pc.FILTER)
        for what, s in defects.items():
            ratio = pc.step_err(s, true) / bar
            print("pose_only/%s/it%d: %s is %.1f bars (%.3g) away" % (name, e, what, ratio, bar))
            within("pose_only/%s/it%d/guard_bars_over_10/%s" % (name, e, what), GUARD_BARS / max(ratio, 1e-12), 1.0)
            if (name, e, what) not in NOT_ACHIEVABLE:
                assert ratio > GUARD_BARS, (name, e, what, ratio)
            else:
                assert ratio > NOT_ACHIEVABLE_FLOOR, (name, e, what, ratio)
