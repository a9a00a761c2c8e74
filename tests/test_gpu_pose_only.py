"""The pose-only refinement (qsp_estimate_pose: k_c0, the Jacobian tiles under the per-hypothesis point mask, the 6 x 6 solve divided by
the number of active points, k_inlier_filter behind iteration index 4) against oracle/sdf_oracle.py:estimate_pose_cam_obj, step by
step.  Cases, step distance and bar: tests/pose_only_cases.py; the conditions under which these tests decide something (no residual
near the filter's threshold, a defective step more than 10 bars away, the yardsticks): tests/test_oracle_pose_only.py.

bar(case, iteration) = max(4 x the float32 oracle's own distance from its float64 evaluation of that step, 1e-4).

* teacher-forced: the library started at the oracle's state before iteration e = 0 .. 4 runs ONE iteration on the full point set;
  and from the state before iteration 5 on the oracle's kept points (a one-iteration call never reaches the filter: the arithmetic
  and the divisor on a compacted set).  1, 31, 33, 63, 64, 65, 129 and 300 points on f32; 1, 33, 64, 65, 129 on bf16x3 and on fp16x2
  with 64- and 32-point tiles; 33 and 65 points of the narrow 4 x 256 / code 32 decoder on f32 and on both fp16x2 tiles.
* the mask path: 5, 6 and 8 free-running iterations on the cases with planted outliers.  The pose stays at the 2e-4 of
  test_gpu_sdf.py; step(pose after 5, pose after 6) meets the oracle's iteration-5 step at the step bar, which a wrong mask or a
  divisor left at the uploaded count cannot (tests/test_oracle_pose_only.py: hundreds of bars).  Five chained one-iteration calls
  are NOT promised to give the bits of one five-iteration call (every call bakes the scale in, inverts, and undoes both on the
  host): their links and their sum are held to the step bar.
* a ragged batch -- 65, 1, 300 with outliers, 64, 33 that the filter empties, 129 points -- in one call: every object's result
  bit for bit its result alone, in reversed order and in a repeated call, at 8 iterations (mask live) and at 1, on f32 and on
  fp16x2 with 32-point tiles.
* the emptied object and an object without points: all 16 entries NaN (include/qsp_hip.h), the neighbours untouched, also when no
  item of the call has a point; refusals leave the output buffer alone.

Every pipe's calls run once per module (fixture `gpu`)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import sdf_oracle as so
from tests import pose_only_cases as pc
from tests.margins import within
from tests.test_oracle_sdf import relerr

pytestmark = pytest.mark.gpu
POSE_BAR = 2e-4            # tests/test_gpu_sdf.py::test_pose_only_more_iterations_exercises_the_inlier_filter
RAGGED_FORMS = (("f32", 64), ("fp16x2", 32))
FREE_ITERS = (5, 6, 8)


def form_id(f):
    return "%s-t%d" % f


def names_on(form):
    """the single cases a form runs"""
    if form == ("f32", 64):
        return pc.SINGLE
    return tuple("m%d" % m for m in pc.PIPE_SIZES) + (tuple("narrow_m%d" % m for m in pc.NARROW_SIZES) if form in pc.NARROW_FORMS else ())


def item(name, start=None, pts=None):
    c = pc.case(name)
    return dict(t_co_se3=c["t_co_se3"] if start is None else start, scale=c["scale"], pts=c["pts"] if pts is None else pts,
                code=c["code"])


@pytest.fixture(scope="module")
def gpu(golden_dir):
    """tag -> array: every library call of this module, pipe by pipe"""
    from qsp_slam_amd import DeepSdfDecoder
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, _estimate_pose
    from tests.test_gpu_sdf import make_cfg
    decs = dict(big=DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz")),
                small=DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_4x256_c32.npz")))
    opts = dict(big=Optimizer(decs["big"], make_cfg(so.JointConfig())), small=Optimizer(decs["small"], make_cfg(so.JointConfig(), code_len=32)))
    out = {}

    def call(which, items, n_iter):
        opts[which].num_iterations_pose_only = n_iter
        return [np.array(T) for T in _estimate_pose(opts[which], decs[which], items, None)]

    try:
        for form in pc.FORMS:
            f = form_id(form)
            for d in decs.values():
                d.set_tile_points(64)
                d.set_precision(form[0])
                d.set_tile_points(form[1])
            out["selected/%s" % f] = np.array([[d.PRECISIONS[d.precision], d.tile_points] for d in decs.values()])
            for name in names_on(form):          # teacher-forced, iterations 0 .. 4
                r = pc.run(name)
                which = r["case"]["decoder"]
                for e in range(5):
                    start = pc.start_of(r["trace"][e]["T_oc"], r["case"]["scale"])
                    out["tf/%s/%s/it%d/start" % (f, name, e)] = start
                    out["tf/%s/%s/it%d/out" % (f, name, e)] = call(which, [item(name, start)], 1)[0]
            for name in pc.FILTER:               # the same from the state before iteration 5 on the kept points, and the mask path
                r = pc.run(name)
                start = pc.start_of(r["trace"][5]["T_oc"], r["case"]["scale"])
                out["tf/%s/%s/it5/start" % (f, name)] = start
                out["tf/%s/%s/it5/out" % (f, name)] = call("big", [item(name, start, pc.points_of(name, 5))], 1)[0]
                for k in FREE_ITERS:
                    out["free/%s/%s/n%d" % (f, name, k)] = call("big", [item(name)], k)[0]
                T = pc.case(name)["t_co_se3"]
                for e in range(5):
                    T = call("big", [item(name, T)], 1)[0]
                    out["chain/%s/%s/after%d" % (f, name, e + 1)] = T
            if form in RAGGED_FORMS:
                for k in (8, 1):
                    items = [item(n) for n in pc.RAGGED]
                    out["ragged/%s/n%d/batch" % (f, k)] = np.stack(call("big", items, k))
                    out["ragged/%s/n%d/repeat" % (f, k)] = np.stack(call("big", items, k))
                    out["ragged/%s/n%d/reversed" % (f, k)] = np.stack(call("big", items[::-1], k)[::-1])
                    out["ragged/%s/n%d/alone" % (f, k)] = np.stack([call("big", [it], k)[0] for it in items])
                    empty = dict(items[1], pts=np.zeros((0, 3), np.float32))      # the same batch with its one-point object given no point
                    out["ragged/%s/n%d/no_points" % (f, k)] = np.stack(call("big", items[:1] + [empty] + items[2:], k))
                out["ragged/%s/emptied_n5" % f] = call("big", [item(pc.EMPTIED)], 5)[0]
        out["range_fallbacks"] = np.array([d.range_fallbacks for d in decs.values()])
    finally:
        for d in decs.values():
            d.close()
    return out


def gpu_step(gpu, tag, name):
    scale = pc.case(name)["scale"]
    return pc.step(pc.T_oc_of(gpu[tag + "/start"], scale), pc.T_oc_of(gpu[tag + "/out"], scale))


def check_step(tag, s, name, e):
    err, bar = pc.step_err(s, pc.oracle_step(name, e)), pc.bar(name, e)
    print("pose_only/%s: step_err %.3g  bar %.3g (yardstick %.3g)  vs the float64 flavour %.3g" % (
        tag, err, bar, pc.yardstick(name, e), pc.step_err(s, pc.oracle_step(name, e, "f64"))))
    return within("pose_only/%s/step_err" % tag, err, bar)


def test_every_form_was_selected_gave_bits_of_its_own_and_none_fell_back(gpu):
    """the library accepted each form's precision and tile size for both decoders, no call was repeated on the f32 pipe, and no
    two forms computed the same bits throughout: of the one-iteration results they share, some differ"""
    from qsp_slam_amd import DeepSdfDecoder
    for form in pc.FORMS:
        assert np.array_equal(gpu["selected/%s" % form_id(form)], [[DeepSdfDecoder.PRECISIONS[form[0]], form[1]]] * 2), form
    assert not gpu["range_fallbacks"].any()
    for i, a in enumerate(pc.FORMS):
        for b in pc.FORMS[i + 1:]:
            fa, fb = "/%s/" % form_id(a), "/%s/" % form_id(b)
            shared = [k for k in gpu if fa in k and k.endswith("/out") and k.replace(fa, fb) in gpu]
            differ = sum(not np.array_equal(gpu[k], gpu[k.replace(fa, fb)]) for k in shared)
            print("pose_only/forms: %s and %s differ in %d of %d shared one-iteration results" % (form_id(a), form_id(b), differ, len(shared)))
            assert len(shared) >= 5 * len(pc.PIPE_SIZES) and differ >= 1, (a, b)


@pytest.mark.parametrize("form", pc.FORMS, ids=form_id)
@pytest.mark.parametrize("e", range(5))
def test_teacher_forced_step(gpu, form, e):
    ok = {}
    for name in names_on(form):
        tag = "tf/%s/%s/it%d" % (form_id(form), name, e)
        ok[name] = check_step(tag, gpu_step(gpu, tag, name), name, e)
    assert all(ok.values()), ok


@pytest.mark.parametrize("form", pc.FORMS, ids=form_id)
@pytest.mark.parametrize("name", pc.FILTER)
def test_teacher_forced_step_behind_the_filter_on_the_kept_points(gpu, form, name):
    assert pc.points_of(name, 5).shape[0] == int(pc.run(name)["kept"].sum()) < pc.case(name)["pts"].shape[0]
    tag = "tf/%s/%s/it5" % (form_id(form), name)
    assert check_step(tag, gpu_step(gpu, tag, name), name, 5)


@pytest.mark.parametrize("form", pc.FORMS, ids=form_id)
@pytest.mark.parametrize("name", pc.FILTER)
def test_free_running_through_the_filter(gpu, form, name):
    f, scale = form_id(form), pc.case(name)["scale"]
    poses = {k: gpu["free/%s/%s/n%d" % (f, name, k)] for k in FREE_ITERS}
    ok = {}
    for k in FREE_ITERS:
        err = relerr(poses[k], pc.oracle_pose(name, k))
        print("pose_only/free/%s/%s/n%d: pose relerr %.3g  bar %.3g" % (f, name, k, err, POSE_BAR))
        ok["pose after %d" % k] = within("pose_only/free/%s/%s/n%d/t_co" % (f, name, k), err, POSE_BAR)
    # the first step on the library's own mask: iteration 5, between its results after 5 and after 6 iterations
    ok["step 5"] = check_step("free/%s/%s/step5" % (f, name), pc.step(pc.T_oc_of(poses[5], scale), pc.T_oc_of(poses[6], scale)), name, 5)
    assert all(ok.values()), ok
    assert relerr(pc.oracle_pose(name, 8), pc.oracle_pose(name, 5)) > 1e-3                 # the filter really changed the trajectory


@pytest.mark.parametrize("form", pc.FORMS, ids=form_id)
@pytest.mark.parametrize("name", pc.FILTER)
def test_five_chained_calls_against_one_call_of_five(gpu, form, name):
    f, c = form_id(form), pc.case(name)
    T = [pc.T_oc_of(c["t_co_se3"], c["scale"])] + [pc.T_oc_of(gpu["chain/%s/%s/after%d" % (f, name, e)], c["scale"]) for e in range(1, 6)]
    ok = [check_step("chain/%s/%s/link%d" % (f, name, e), pc.step(T[e], T[e + 1]), name, e) for e in range(5)]
    whole = pc.step(T[0], pc.T_oc_of(gpu["free/%s/%s/n5" % (f, name)], c["scale"]))
    err, bar = pc.step_err(pc.step(T[0], T[5]), whole), max(pc.bar(name, e) for e in range(5))
    print("pose_only/chain/%s/%s: five calls against one call of five, step_err %.3g  bar %.3g" % (f, name, err, bar))
    assert within("pose_only/chain/%s/%s/whole" % (f, name), err, bar) and all(ok), ok


@pytest.mark.parametrize("form", RAGGED_FORMS, ids=form_id)
@pytest.mark.parametrize("k", (8, 1))
def test_ragged_batch_gives_every_object_its_alone_bits(gpu, form, k):
    tag = "ragged/%s/n%d/" % (form_id(form), k)
    alone = gpu[tag + "alone"]
    i_empty = pc.RAGGED.index(pc.EMPTIED)
    for i, name in enumerate(pc.RAGGED):
        assert np.isfinite(alone[i]).all() == (k == 1 or i != i_empty), name
    for what in ("batch", "repeat", "reversed"):
        for i, name in enumerate(pc.RAGGED):
            assert np.array_equal(gpu[tag + what][i], alone[i], equal_nan=True), (what, name)


@pytest.mark.parametrize("form", RAGGED_FORMS, ids=form_id)
def test_an_object_without_a_point_left_is_all_nan_and_its_neighbours_keep_their_bits(gpu, form):
    """pinned: include/qsp_hip.h, qsp_estimate_pose.  The oracle divides by zero there and returns a non-finite pose
    (tests/test_oracle_pose_only.py); the pose the hypothesis had when it stopped is not handed out as a result."""
    f = form_id(form)
    i_empty = pc.RAGGED.index(pc.EMPTIED)
    assert np.isnan(gpu["ragged/%s/n8/alone" % f][i_empty]).all() and np.isnan(gpu["ragged/%s/n8/batch" % f][i_empty]).all()
    five = gpu["ragged/%s/emptied_n5" % f]                  # five iterations never reach the filter: a finite matrix
    assert np.isfinite(five).all()
    for k in (8, 1):                                        # n_pts[1] = 0: that item NaN at any iteration count, the others as alone
        got, alone = gpu["ragged/%s/n%d/no_points" % (f, k)], gpu["ragged/%s/n%d/alone" % (f, k)]
        assert np.isnan(got[1]).all()
        for i in range(len(pc.RAGGED)):
            if i != 1:
                assert np.array_equal(got[i], alone[i], equal_nan=True), (k, pc.RAGGED[i])


def test_refusals_leave_the_output_buffer_untouched(gpu, golden_dir):
    from qsp_slam_amd import DeepSdfDecoder, _lib
    L = _lib.lib()
    d = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz"))
    try:
        cs = [pc.case("m33"), pc.case("m1")]
        T = _lib.f32c(np.stack([c["t_co_se3"].reshape(16) for c in cs]))
        sc = np.array([c["scale"] for c in cs], np.float32)
        ps = [_lib.f32c(c["pts"]) for c in cs]
        code = _lib.f32c(np.stack([c["code"] for c in cs]))
        sentinel = np.float32(-7.25)

        def call(n, pts_ptrs, n_pts):
            out = np.full((2, 4, 4), sentinel, np.float32)
            rc = L.qsp_estimate_pose(d.handle, n, _lib.fptr(T), _lib.fptr(sc), C.cast(pts_ptrs, C.POINTER(_lib.c_float_p)),
                                     _lib.i32ptr(np.array(n_pts, np.int32)), _lib.fptr(code), 5, _lib.fptr(out))
            return rc, out
        good = _lib.ptr_array(ps)
        with_null = (_lib.c_float_p * 2)(_lib.fptr(ps[0]), _lib.c_float_p())
        for what, args in (("n = 0", (0, good, [33, 1])), ("a null pts entry", (2, with_null, [33, 1])),
                           ("a negative n_pts", (2, good, [33, -1]))):
            rc, out = call(*args)
            assert rc == _lib.QSP_ERR_INVALID and b"qsp_estimate_pose" in L.qsp_last_error(), what
            assert (out == sentinel).all(), what
        rc, out = call(2, with_null, [33, 0])                # a null entry is not read when its count is 0
        assert rc == _lib.QSP_OK and np.isfinite(out[0]).all() and np.isnan(out[1]).all()
        for n, n_pts in ((1, [0, 0]), (2, [0, 0])):          # no item has a point: nothing is launched, every item NaN
            rc, out0 = call(n, with_null if n == 2 else good, n_pts)
            assert rc == _lib.QSP_OK and np.isnan(out0[:n]).all() and (out0[n:] == sentinel).all(), n
        rc, ref = call(2, good, [33, 1])
        assert rc == _lib.QSP_OK and np.isfinite(ref).all() and np.array_equal(ref[0], out[0])
    finally:
        d.close()
