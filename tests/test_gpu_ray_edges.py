"""The ray-sample list kernels of the render term (csrc/sdf_kernels.hpp: k_sample, k_scan, k_stage_list, the plan tails) beyond one
pass of rays and off 50 depth samples, against oracle/sdf_oracle.py on the cases of tests/ray_edges.py: 511 .. 1537 rays (the second
and later passes of k_scan with its table clear and `(e >> 6) - base` row index, the second pass of k_sample, up to seven of
k_stage_list, the offsets each carries from pass to pass), D = 3, 4, 5, 7, 49, 63, 64 (bit 62 of the sample masks, the full row of
the LDS table, k_mid = D // 2 rounding down, the first staged counts), and the reference's exits: fewer than 10 valid samples, no
rays at all, valid samples but no kept row (K = 0, optimizer.py:193-194), a depth count outside 2 .. 64.

Bars: n_valid and K exact (the seeds keep every threshold decision out of rounding's reach, tests/test_ray_edge_cases.py); column 71
of every render row at 1e-4 of its largest value with no row excused (it comes from the forward pass alone and ties the row to its
ray's observed and rendered depth, so to the row order); Jacobian rows at the bars of
tests/test_gpu_sdf.py::test_jacobian_rows_of_fused_kernel_vs_reference, per group of rows (the k_scan pass of the ray; the depth
stage of the sample) and with no row out of a group of fewer than 50 -- a wrong last pass of two rows must not hide inside 2 % of
500; H, b and the two losses at the 1e-4 of test_one_iteration_vs_oracle_other_sizes.  Screened and depth-staged runs equal the
one-pass run bit for bit.  Every figure is printed before it is asserted, and a run with QSP_MARGINS_OUT lists it under
`ray_edges/<case>/<pipe>/`."""
import os

import numpy as np
import pytest

from oracle import sdf_oracle as so
from tests import ray_edges as re_
from tests.margins import within
from tests.test_gpu_screening import assert_same_bits, run_batch
from tests.test_gpu_sdf import make_cfg
from tests.test_oracle_sdf import relerr

pytestmark = pytest.mark.gpu
PIPES = ("f32", "fp16x2")


@pytest.fixture(scope="module")
def dec(golden_dir):
    from qsp_slam_amd import DeepSdfDecoder
    d = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz"))
    yield d
    d.close()


def set_pipe(dec, pipe):
    """the f32 pipe, or the split-fp16 pipe unscreened: one pass over every valid sample"""
    dec.set_precision(pipe)
    if pipe == "fp16x2":
        dec.set_render_screening(0.0)


def new_batch(dec, cfg, objs, hyp=None):
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, RefineBatch, _joint_cfg
    return RefineBatch(dec, _joint_cfg(Optimizer(dec, make_cfg(cfg))), [o["pts"] for o in objs], [o["rays"] for o in objs],
                       [o["depth"] for o in objs], list(range(len(objs))) if hyp is None else hyp)


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("name", list(re_.CASES))
def test_one_iteration_vs_the_oracle(dec, name, pipe):
    """one teacher-forced iteration from t_cam_obj, rows enabled"""
    case = re_.build_case(name)
    it, rt, cfg, o = case["it"], case["rt"], case["cfg"], case["obj"]
    set_pipe(dec, pipe)
    n_fb = dec.range_fallbacks
    b = new_batch(dec, cfg, [o])
    b.enable_rows(True)
    b.set_state(case["T0"], None)
    b.run(1)
    tr = b.trace()
    T, code, loss, good = b.get()
    n_valid, K = int(tr["n_valid"][0]), int(tr["K"][0])
    rr = b.rows(0, re_.M_PTS, K)[1] if K > 0 else np.zeros((0, 72), np.float32)
    b.close()
    assert dec.range_fallbacks == n_fb                   # the pipe under test is the one that ran
    print("ray_edges/%s/%s: n_valid %d (oracle %d) K %d (oracle %d)" % (name, pipe, n_valid, it["n_valid"], K, it["K"]))
    assert it["fail"] is None and bool(good[0])
    assert n_valid == it["n_valid"] and K == it["K"]
    tag = "ray_edges/%s/%s/" % (name, pipe)
    # column 71: the robust residual of every row, none excused
    rob = so.robust_residual(it["res_render"], cfg.b1)[0]
    res_err = np.abs(rr[:, 71].astype(np.float64) - rob) / np.abs(rob).max()
    # columns 0..70, per group of rows
    groups, n_groups = re_.row_groups(case)
    err = re_.jacobian_row_errors(rr[:, :7], rr[:, 7:71], it)
    rows_ok, rows_worst, rows_small = re_.grouped_rows_ok(err, groups, n_groups)
    fig = dict(res71=float(res_err.max()), rows_worst=rows_worst, rows_small_groups=rows_small,
               rows_out=[int((err[groups == g] > re_.ROW_TOL).sum()) for g in range(n_groups)],
               rows_per_group=[int((groups == g).sum()) for g in range(n_groups)],
               H=relerr(tr["H"][0], it["H"]), b=relerr(tr["b"][0], it["b"]),
               loss_sdf=abs(float(tr["loss_sdf"][0]) - it["loss_sdf"]) / it["loss_sdf"],
               loss_render=abs(float(tr["loss_render"][0]) - it["loss_render"]) / it["loss_render"])
    print("ray_edges/%s/%s: %s" % (name, pipe, fig))
    ok = [within(tag + "res71", fig["res71"], re_.RES_TOL),
          within(tag + "rows_small_groups", fig["rows_small_groups"], re_.ROW_TOL),
          within(tag + "rows_out_share", max([n_out / max(n, 1) for n_out, n in zip(fig["rows_out"], fig["rows_per_group"])
                                               if n >= re_.SMALL_GROUP], default=0.0), re_.ROW_MAX_BAD),
          within(tag + "H", fig["H"], 1e-4), within(tag + "b", fig["b"], 1e-4),
          within(tag + "loss_sdf_rel", fig["loss_sdf"], 1e-4), within(tag + "loss_render_rel", fig["loss_render"], 1e-4)]
    assert rows_ok and all(ok), fig


@pytest.mark.parametrize("name", re_.STAGED)
def test_screened_and_depth_staged_runs_equal_the_one_pass_run_bit_for_bit(dec, name):
    """three free-running iterations on the split-fp16 pipe: unscreened, screened in one depth stage, screened in two (D = 3 is
    below the staging threshold and simply equals the others); the staged run evaluates fewer samples wherever the oracle has an
    opaque sample in front of k_mid on a ray that goes on behind it"""
    from qsp_slam_amd.reconstruct.optimizer import Optimizer
    case = re_.build_case(name)
    opt = Optimizer(dec, make_cfg(so.JointConfig(n_iter=3, n_depth=case["D"])))
    dec.set_precision("fp16x2")
    try:
        dec.set_screening_min_samples(0)
        one_pass = run_batch(dec, opt, [case["obj"]], [0], case["T0"], None, 3, False)
        dec.set_depth_staging(False)
        flat = run_batch(dec, opt, [case["obj"]], [0], case["T0"], None, 3, True)
        dec.set_depth_staging("always")
        staged = run_batch(dec, opt, [case["obj"]], [0], case["T0"], None, 3, True)
    finally:
        dec.set_depth_staging(True)
        dec.set_render_screening(0.0)
        dec.set_screening_min_samples(-1)
    skipped = re_.opaque_before_mid(case)
    print("ray_edges/%s/staging: pts_fwd one pass %d, screened %d, staged %d; band %d / %d; oracle: %d samples behind an opaque one"
          % (name, one_pass["prof"].pts_fwd, flat["prof"].pts_fwd, staged["prof"].pts_fwd, flat["prof"].pts_band,
             staged["prof"].pts_band, skipped))
    assert int(one_pass["n_valid"][0]) > 0
    assert_same_bits(one_pass, flat, name + ": screened, one depth stage")
    assert_same_bits(one_pass, staged, name + ": screened, two depth stages")
    for out in (flat, staged):
        assert out["prof"].screen_fallbacks == 0 and out["prof"].pts_band > 0       # (the screened form is the one that ran)
    assert one_pass["prof"].pts_band == 0 and flat["prof"].pts_fwd == one_pass["prof"].pts_fwd
    assert staged["prof"].pts_fwd <= flat["prof"].pts_fwd
    if case["D"] < 4:
        assert staged["prof"].pts_fwd == flat["prof"].pts_fwd
    elif skipped > 0:
        assert staged["prof"].pts_fwd < flat["prof"].pts_fwd


@pytest.mark.parametrize("pipe", PIPES)
def test_one_ragged_batch_equals_its_single_object_batches(dec, pipe):
    """objects of 0, 40, 513 and 1025 rays in one batch, a hypothesis each, two iterations: every hypothesis walks its own number of
    passes beside the others and equals its own single-object batch bit for bit"""
    objs = re_.ragged_objects()
    assert re_.RAGGED == (0, 40, 513, 1025) and all(o["pts"].shape == (re_.M_PTS, 3) for o in objs)
    cfg = so.JointConfig(n_iter=2)
    set_pipe(dec, pipe)

    def run(sub):
        b = new_batch(dec, cfg, sub)
        b.set_state(np.stack([o["t_cam_obj"] for o in sub]), None)
        b.run(2)
        out = dict(zip(("T", "code", "loss", "good"), b.get()))
        out.update(K=b.trace()["K"], n_valid=b.trace()["n_valid"])
        b.close()
        return out

    ragged = run(objs)
    print("ray_edges/ragged/%s: good %s loss %s K %s n_valid %s" % (pipe, ragged["good"], ragged["loss"], ragged["K"], ragged["n_valid"]))
    assert not ragged["good"][0] and float(ragged["loss"][0]) == 0.0 and int(ragged["n_valid"][0]) == 0
    assert ragged["good"][1:].all() and (ragged["K"][1:] > 0).all()
    for h, o in enumerate(objs):
        single = run([o])
        for k in ("T", "code", "loss", "good", "K", "n_valid"):
            assert np.array_equal(ragged[k][h], single[k][0], equal_nan=True), (h, k)


@pytest.mark.parametrize("pipe", PIPES)
def test_exits_are_the_references(dec, pipe):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.reconstruct.optimizer import Optimizer
    set_pipe(dec, pipe)
    # fewer than 10 valid samples (D = 2: both samples of every ray lie on the unit sphere), and no rays at all
    n_fg, n_bg, D, seed = re_.NONE_CASE
    o = re_.make_object(seed, n_fg, n_bg)
    for obj, cfg in ((o, so.JointConfig(n_depth=D)), (re_.no_ray_object(), so.JointConfig())):
        r = Optimizer(dec, make_cfg(cfg)).reconstruct_object(obj["t_cam_obj"], obj["pts"], obj["rays"], obj["depth"])
        assert r.is_good is False and r.t_cam_obj is None and r.code is None and r.loss == 0.0
    # valid samples, but no kept render row: mean over an empty set is NaN (optimizer.py:193-194)
    n_fg, n_bg, D, seed, n_pts = re_.NAN_CASE
    c = re_.build(n_fg, n_bg, D, seed, n_pts)
    assert c["it"]["fail"] == "render_nan"
    b = new_batch(dec, c["cfg"], [c["obj"]])
    b.set_state(c["T0"], None)
    b.run(1)
    tr, (T, code, loss, good) = b.trace(), b.get()
    b.close()
    print("ray_edges/render_nan/%s: n_valid %d (oracle %d) K %d good %s" % (pipe, tr["n_valid"][0], c["it"]["n_valid"], tr["K"][0], good[0]))
    assert not good[0] and int(tr["n_valid"][0]) == c["it"]["n_valid"] >= 10 and int(tr["K"][0]) == 0 and float(loss[0]) == 0.0
    r = Optimizer(dec, make_cfg(c["cfg"])).reconstruct_object(c["obj"]["t_cam_obj"], c["obj"]["pts"], c["obj"]["rays"], c["obj"]["depth"])
    assert r.is_good is False and r.t_cam_obj is None and r.loss == 0.0
    # a depth count the packed index (ray << 6) | k and the 64-bit masks cannot hold, or that has no depth step
    for D in (1, 65):
        opt = Optimizer(dec, make_cfg(so.JointConfig(n_depth=D)))
        with pytest.raises(_lib.QspError) as e:
            new_batch(dec, so.JointConfig(n_depth=D), [o])
        assert e.value.code == _lib.QSP_ERR_INVALID
        with pytest.raises(_lib.QspError) as e:
            opt.reconstruct_object(o["t_cam_obj"], o["pts"], o["rays"], o["depth"])
        assert e.value.code == _lib.QSP_ERR_INVALID
