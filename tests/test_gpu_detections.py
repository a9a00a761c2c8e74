"""GPU parity of qsp_refine_detections (the caller-side marshalling of path A on the device,
reference src/LocalMapping_util.cc:585-760) through the C-ABI.

  * the assembled inputs (camera-frame surface points, rays, observed depths, flip initial poses) equal the restatement in
    oracle/detections_oracle.py BIT FOR BIT.  Tolerance against a build of the reference itself: its OpenCV / Eigen may
    contract a*b+c into an FMA (-march=native), which moves a ray or pose entry by at most 1 ulp (6e-8 relative); the refined
    poses are insensitive to that at the 1e-4 level north_star asks for;
  * the refinement that follows is the SAME arithmetic as the host-fed batch: every hypothesis equals, to the bit, the result of
    Optimizer.reconstruct_object on the oracle-assembled inputs (that entry point is pinned against the reference's golden
    vectors in tests/test_gpu_sdf.py);
  * the kept result is the one the reference's keep rule selects (oracle keep_rule), including not-good hypotheses, detections
    that already have a good orientation (one hypothesis), ragged and empty inputs.

The edge cases behind the first four tests use tests/detection_cases.py: intrinsics that differ per detection, the second pass of
k_det_assemble's grid-stride loops beside a small neighbour, a middle flip kept on its loss, a code of 32, 64 flips, detections
without feature points or without map points, and the C ABI built by hand: its optional arguments and every refusal."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import bench
from oracle import detections_oracle as DO
from qsp_slam_amd import synth
from tests import detection_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_decoder(golden_dir):
    from qsp_slam_amd import DeepSdfDecoder
    d = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz"))
    yield d
    d.close()


def _optimizer(gpu_decoder, n_iter=3):
    from qsp_slam_amd.reconstruct.optimizer import Optimizer
    return Optimizer(gpu_decoder, bench.joint_cfg(n_iter))


def _check_against_oracle(opt, dets, flips, res):
    ang = 2.0 * math.pi / flips
    for d, r in zip(dets, res):
        nf = 1 if d.get("found_good_orientation") else flips
        pts, rays, depth = DO.assemble(d)
        T0 = DO.init_poses(d, nf, ang)
        assert np.array_equal(r.pts, pts) and np.array_equal(r.rays, rays) and np.array_equal(r.depth, depth)
        assert np.array_equal(r.t_cam_obj_init, T0)
        singles = [opt.reconstruct_object(T0[k], pts, rays, depth, d.get("code")) for k in range(nf)]
        good = [s.is_good for s in singles]
        loss = [np.float32(s.loss) for s in singles]
        assert np.array_equal(np.asarray(r.losses, np.float32), np.asarray(loss, np.float32), equal_nan=True)
        k = DO.keep_rule(good, loss)
        assert r.kept_flip == k and r.is_good == good[k]
        if good[k]:
            assert np.array_equal(r.t_cam_obj, singles[k].t_cam_obj) and np.array_equal(r.code, singles[k].code)
            assert np.float32(r.loss) == loss[k]
        else:
            assert r.t_cam_obj is None and r.code is None


def test_detections_match_oracle_assembly_and_serial_calls(gpu_decoder):
    opt = _optimizer(gpu_decoder)
    dets = synth.make_detections(11, 5, 700, n_fg=96, n_bg=40, n_kf=2)
    dets[3]["found_good_orientation"] = True
    dets[4]["code"] = (0.05 * np.random.default_rng(0).normal(size=64)).astype(np.float32)
    res = opt.refine_detections(dets, flip_sample_num=4, taps=True)
    _check_against_oracle(opt, dets, 4, res)
    # the un-flipped start is the perturbed ground truth: it is kept unless a flip is better by the rule, and it moved closer
    assert all(r.is_good for r in res)


def test_detections_ragged_empty_and_failing(gpu_decoder):
    """ragged counts, a detection whose rays all miss the object (fewer than 10 samples in the unit ball -> every
    hypothesis not good -> the LAST one is kept by the rule and t_cam_obj is None), six flips"""
    opt = _optimizer(gpu_decoder, n_iter=2)
    dets = synth.make_detections(12, 3, 300, n_fg=48, n_bg=16)
    dets[0]["pts_world"] = dets[0]["pts_world"][:37]
    dets[1]["bg_rays"] = dets[1]["bg_rays"][:0]
    far = dets[2]
    far["fg_px"] = far["fg_px"] + np.float32(4000.0)            # rays that never enter the unit ball
    far["bg_rays"] = far["bg_rays"] + np.float32(9.0)
    res = opt.refine_detections(dets, flip_sample_num=6, taps=True)
    _check_against_oracle(opt, dets, 6, res)
    assert not res[2].is_good and res[2].kept_flip == 5 and res[2].t_cam_obj is None
    assert res[0].is_good and res[1].is_good


def test_detections_argument_errors(gpu_decoder):
    from qsp_slam_amd import _lib
    opt = _optimizer(gpu_decoder)
    d = synth.make_detections(13, 1, 50, n_fg=16, n_bg=4)[0]
    bad = dict(d)
    bad["fg_world"] = d["fg_world"][:-1]
    with pytest.raises(ValueError):
        opt.refine_detections([bad])
    with pytest.raises(_lib.QspError):
        opt.refine_detections([d], flip_sample_num=65)


def test_detections_c4_sized_call_equals_host_fed_batch(gpu_decoder):
    """64 detections x 4 flips x 8 k points in one call (the C4 batch) == RefineBatch fed with the oracle-assembled arrays"""
    from qsp_slam_amd.reconstruct.optimizer import RefineBatch, _joint_cfg
    w = bench.WORKLOADS["c4"]
    opt = _optimizer(gpu_decoder, n_iter=2)
    dets = synth.make_detections(14, 64, w["n_pts"], n_fg=w["n_fg"], n_bg=w["n_bg"], n_kf=5)
    res = opt.refine_detections(dets, flip_sample_num=4)
    asm = [DO.assemble(d) for d in dets]
    T0 = np.concatenate([DO.init_poses(d, 4, 2.0 * math.pi / 4) for d in dets])
    hyp = np.repeat(np.arange(64), 4)
    batch = RefineBatch(gpu_decoder, _joint_cfg(opt), [a[0] for a in asm], [a[1] for a in asm], [a[2] for a in asm], hyp)
    batch.set_state(T0, None)
    batch.run(0)
    T, code, loss, good = batch.get()
    batch.close()
    for i, r in enumerate(res):
        k = DO.keep_rule(list(good[4 * i:4 * i + 4]), list(loss[4 * i:4 * i + 4]))
        assert r.kept_flip == k and np.array_equal(r.losses, loss[4 * i:4 * i + 4])
        assert np.array_equal(r.t_cam_obj, T[4 * i + k]) and np.array_equal(r.code, code[4 * i + k])


# ---- edges and refusals (tests/detection_cases.py) ----------------------------------------------------------------------------

def _n_flip(dets, flips):
    return [1 if d.get("found_good_orientation") else flips for d in dets]


def _host_fed(decoder, opt, dets, flips):
    """RefineBatch fed with the oracle-assembled arrays and initial poses: per detection (T, code, loss, good) of its hypotheses"""
    from qsp_slam_amd.reconstruct.optimizer import RefineBatch, _joint_cfg
    nf = _n_flip(dets, flips)
    asm = [DO.assemble(d) for d in dets]
    T0 = np.concatenate([DO.init_poses(d, k, 2.0 * math.pi / flips) for d, k in zip(dets, nf)])
    hyp = np.repeat(np.arange(len(dets)), nf)
    codes = None
    if any(d.get("code") is not None for d in dets):
        rows = [np.zeros(opt.code_len, np.float32) if d.get("code") is None else np.asarray(d["code"], np.float32)[:opt.code_len]
                for d in dets]
        codes = np.stack([rows[i] for i in hyp])
    batch = RefineBatch(decoder, _joint_cfg(opt), [a[0] for a in asm], [a[1] for a in asm], [a[2] for a in asm], hyp)
    batch.set_state(T0, codes)
    batch.run(0)
    T, code, loss, good = batch.get()
    batch.close()
    off = np.concatenate([[0], np.cumsum(nf)])
    return [(T[a:b], code[a:b], loss[a:b], good[a:b]) for a, b in zip(off[:-1], off[1:])]


def _check_against_host_fed(decoder, opt, dets, flips, res):
    """the taps against the oracle, every loss and the kept result against the host-fed batch of the same shape"""
    ang = 2.0 * math.pi / flips
    for i, (d, r, (T, code, loss, good)) in enumerate(zip(dets, res, _host_fed(decoder, opt, dets, flips))):
        pts, rays, depth = DO.assemble(d)
        assert np.array_equal(r.pts, pts), i
        assert np.array_equal(r.rays, rays), i
        assert np.array_equal(r.depth, depth), i
        assert np.array_equal(r.t_cam_obj_init, DO.init_poses(d, len(loss), ang)), i
        assert np.array_equal(r.losses, loss, equal_nan=True), i
        k = DO.keep_rule(list(good), list(loss))
        assert r.kept_flip == k and r.is_good == bool(good[k]), i
        if good[k]:
            assert np.array_equal(r.t_cam_obj, T[k]) and np.array_equal(r.code, code[k]) and np.float32(r.loss) == loss[k], i
        else:
            assert r.t_cam_obj is None and r.code is None, i


def test_detections_with_their_own_intrinsics(gpu_decoder):
    """four detections through four cameras (fx != fy, distinct principal points): K is indexed by the detection"""
    opt = _optimizer(gpu_decoder, n_iter=2)
    dets = [dc.with_intrinsics(d, K) for d, K in zip(synth.make_detections(11, 4, 700, n_fg=96, n_bg=40, n_kf=2), dc.INTRINSICS)]
    assert len({d["K"].tobytes() for d in dets}) == 4
    res = opt.refine_detections(dets, flip_sample_num=4, taps=True)
    _check_against_oracle(opt, dets, 4, res)
    assert all(r.is_good for r in res)


def test_detections_second_stride_pass_beside_small_neighbours(gpu_decoder):
    """k_det_assemble runs at most 64 x 256 threads per detection: 16385 map points, 16385 feature points and 16386 background
    floats take the `i += stride` pass of its three loops, 16384 points stop short of it, and the 37-point detections at both ends
    of the call run under the same 64 blocks"""
    opt = _optimizer(gpu_decoder, n_iter=1)
    dets = dc.stride_detections()
    assert [len(d["pts_world"]) for d in dets] == [37, 16385, 64, 64, 16384, 37]
    assert len(dets[2]["fg_px"]) == 16385 and 3 * len(dets[3]["bg_rays"]) == 16386
    res = opt.refine_detections(dets, flip_sample_num=4, taps=True)
    _check_against_host_fed(gpu_decoder, opt, dets, 4, res)
    assert [len(r.losses) for r in res] == [4, 1, 1, 1, 1, 4]


@pytest.mark.parametrize("name", sorted(dc.MIDDLE_FLIP))
def test_detections_keep_a_middle_flip_on_its_loss(gpu_decoder, name):
    """Sim3Two turned k flips back (detection_cases.with_yaw): hypothesis k starts at the perturbed ground truth and is kept
    because its loss is the smallest -- neither the first nor the last of the good ones (the gap is asserted on the CPU,
    tests/test_oracle_detections.py)"""
    flips, n_iter, _, _, yaws = dc.MIDDLE_FLIP[name]
    opt = _optimizer(gpu_decoder, n_iter=n_iter)
    dets = dc.middle_flip_detections(name)
    res = opt.refine_detections(dets, flip_sample_num=flips, taps=True)
    _check_against_oracle(opt, dets, flips, res)
    assert [r.kept_flip for r in res] == [k or 0 for k in yaws]
    assert all(r.is_good for r in res)
    assert any(0 < r.kept_flip < flips - 1 for r in res)


@pytest.fixture(scope="module")
def small_gpu_decoder(golden_dir):
    from qsp_slam_amd import DeepSdfDecoder
    d = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_4x256_c32.npz"))
    yield d
    d.close()


def test_detections_code_length_32(small_gpu_decoder):
    """the 4 x 256 decoder with a code of 32: `code` goes in and comes out in rows of 32 while the hypothesis state holds 64"""
    from qsp_slam_amd.reconstruct.optimizer import Optimizer
    cfg = bench.joint_cfg(2)
    cfg.optimizer.code_len = 32
    opt = Optimizer(small_gpu_decoder, cfg)
    assert small_gpu_decoder.code_len == 32
    dets = synth.make_detections(16, 3, 300, n_fg=48, n_bg=16)
    dets[0]["code"] = None
    for i in (1, 2):
        dets[i]["code"] = (0.05 * np.random.default_rng(160 + i).normal(size=32)).astype(np.float32)
    res = opt.refine_detections(dets, flip_sample_num=4, taps=True)
    _check_against_oracle(opt, dets, 4, res)
    assert all(r.is_good and r.code.shape == (32,) for r in res)
    assert len({r.code.tobytes() for r in res}) == 3


def test_detections_64_flips(gpu_decoder):
    """the bound of n_flip: one thread per flip of k_det_init's 64-thread block, a Ry table of 64 rotations, beside a detection
    with one hypothesis"""
    opt = _optimizer(gpu_decoder, n_iter=1)
    dets = synth.make_detections(17, 2, 60, n_fg=16, n_bg=6)
    dets[1]["found_good_orientation"] = True
    res = opt.refine_detections(dets, flip_sample_num=64, taps=True)
    assert res[0].t_cam_obj_init.shape == (64, 4, 4) and res[1].t_cam_obj_init.shape == (1, 4, 4)
    assert len({T.tobytes() for T in res[0].t_cam_obj_init}) == 64
    _check_against_host_fed(gpu_decoder, opt, dets, 64, res)


def test_detections_without_feature_points_or_map_points(gpu_decoder):
    """n_fg == 0: the rays are the background rays alone and nothing of the detection goes into depth_obs, whose compaction on the
    host skips it -- the neighbours' observed depths stay theirs.  n_pts == 0: accepted; the SDF term's mean over no point is NaN,
    so every hypothesis ends not good with loss 0 (optimizer.py:168-169) and the last one is kept, as the serial call gives."""
    opt = _optimizer(gpu_decoder, n_iter=2)
    dets = synth.make_detections(18, 4, 120, n_fg=32, n_bg=12)
    dets[1] = dc.with_counts(dets[1], n_fg=0)
    dets[3] = dc.with_counts(dets[3], n_pts=0)
    assert dets[1]["fg_px"].shape == (0, 2) and dets[1]["fg_world"].shape == (0, 3) and dets[3]["pts_world"].shape == (0, 3)
    res = opt.refine_detections(dets, flip_sample_num=4, taps=True)
    _check_against_oracle(opt, dets, 4, res)
    _check_against_host_fed(gpu_decoder, opt, dets, 4, res)
    assert res[1].depth.shape == (0,) and res[1].rays.shape == (12, 3)
    assert res[0].is_good and res[2].is_good
    assert not res[3].is_good and res[3].kept_flip == 3 and res[3].loss == 0.0 and not res[3].losses.any()
    # no map points anywhere in the call
    lone = [dc.with_counts(d, n_pts=0) for d in dets[:2]]
    r2 = opt.refine_detections(lone, flip_sample_num=2, taps=True)
    _check_against_oracle(opt, lone, 2, r2)
    assert not any(r.is_good for r in r2) and all(r.pts.shape == (0, 3) for r in r2)


# ---- the C ABI, built by hand -------------------------------------------------------------------------------------------------

_IN = ("T_cw", "K", "T_wo", "code", "n_flip", "pts_off", "pts_world", "fg_off", "fg_px", "fg_world", "bg_off", "bg_rays")
_OUT = ("t_cam_obj", "code", "loss", "is_good", "kept_flip", "losses", "pts_cam", "rays", "depth_obs", "t_cam_obj_init")


def _raw(dets, flips, code_len=64, with_n_flip=True):
    """the arrays of a call, built by hand so that single fields can be broken: (inputs, sentinel-filled outputs)"""
    n = len(dets)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    a = dict(T_cw=f32(np.stack([d["T_cw"] for d in dets])), K=f32(np.stack([d["K"] for d in dets])),
             T_wo=f32(np.stack([d["T_wo"] for d in dets])),
             code=f32(np.stack([np.zeros(code_len) if d.get("code") is None else d["code"][:code_len] for d in dets])),
             n_flip=np.array(_n_flip(dets, flips), np.int32))
    for key, off, w in (("pts_world", "pts_off", 3), ("fg_px", "fg_off", 2), ("fg_world", "fg_off", 3), ("bg_rays", "bg_off", 3)):
        a[off] = np.concatenate([[0], np.cumsum([len(d[key]) for d in dets])]).astype(np.int32)
        a[key] = f32(np.concatenate([np.asarray(d[key]).reshape(-1, w) for d in dets]))
    n_hyp = int(a["n_flip"].sum()) if with_n_flip else n
    n_p, n_f, n_b = int(a["pts_off"][-1]), int(a["fg_off"][-1]), int(a["bg_off"][-1])
    s = np.float32(-7.0)
    o = dict(t_cam_obj=np.full((n, 4, 4), s), code=np.full((n, code_len), s), loss=np.full(n, s), is_good=np.full(n, 9, np.uint8),
             kept_flip=np.full(n, -5, np.int32), losses=np.full(n_hyp, s), pts_cam=np.full((n_p, 3), s), rays=np.full((n_f + n_b, 3), s),
             depth_obs=np.full(n_f, s), t_cam_obj_init=np.full((n_hyp, 4, 4), s))
    return a, o


def _call(handle, cfg, a, o, flips, drop=(), det_class=None, n_det=None, **changed):
    """qsp_refine_detections (det_class None) or its group form on hand-built structs: `drop` names the pointers passed as NULL,
    `changed` replaces input arrays"""
    from qsp_slam_amd import _lib
    ptr = {np.dtype(np.float32): _lib.fptr, np.dtype(np.int32): _lib.i32ptr, np.dtype(np.uint8): _lib.u8ptr}
    a = dict(a, **changed)
    p = lambda d, k: None if k in drop else ptr[d[k].dtype](d[k])
    inp = _lib.Detections(len(a["T_cw"]) if n_det is None else n_det, p(a, "T_cw"), p(a, "K"), p(a, "T_wo"), p(a, "code"),
                          p(a, "n_flip"), 2.0 * math.pi / flips, p(a, "pts_off"), p(a, "pts_world"), p(a, "fg_off"), p(a, "fg_px"),
                          p(a, "fg_world"), p(a, "bg_off"), p(a, "bg_rays"))
    out = _lib.DetectionResults(*[None if ("out_" + k) in drop else ptr[o[k].dtype](o[k]) for k in _OUT])
    if det_class is None:
        return _lib.lib().qsp_refine_detections(handle, C.byref(cfg), C.byref(inp), C.byref(out))
    cls = np.ascontiguousarray(det_class, dtype=np.int32)
    return _lib.lib().qsp_refine_detections_group(handle, C.byref(cfg), C.byref(inp), _lib.i32ptr(cls), C.byref(out))


def _tiny(code=True):
    dets = synth.make_detections(19, 2, 60, n_fg=32, n_bg=6)
    if code:
        dets[1]["code"] = (0.05 * np.random.default_rng(19).normal(size=64)).astype(np.float32)
    return dets


def test_c_abi_optional_arguments(gpu_decoder):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.reconstruct.optimizer import _joint_cfg
    opt = _optimizer(gpu_decoder, n_iter=1)
    cfg, h = _joint_cfg(opt), gpu_decoder.handle
    dets = _tiny()
    # n_flip == NULL: one hypothesis each, as the wrapper's call with found_good_orientation everywhere
    a, o = _raw(dets, 4, with_n_flip=False)
    assert _call(h, cfg, a, o, 4, drop=("n_flip",)) == _lib.QSP_OK
    ref = opt.refine_detections([dict(d, found_good_orientation=True) for d in dets], flip_sample_num=4, taps=True)
    assert ref[0].is_good and not o["kept_flip"].any()
    for i, r in enumerate(ref):
        assert bool(o["is_good"][i]) == r.is_good
        if r.is_good:
            assert np.array_equal(o["t_cam_obj"][i], r.t_cam_obj) and np.array_equal(o["code"][i], r.code)
        assert o["loss"][i] == np.float32(r.loss) and np.array_equal(o["losses"][i:i + 1], r.losses)
        assert np.array_equal(o["t_cam_obj_init"][i:i + 1], r.t_cam_obj_init)
    assert np.array_equal(o["pts_cam"], np.concatenate([r.pts for r in ref]))
    assert np.array_equal(o["rays"], np.concatenate([r.rays for r in ref]))
    assert np.array_equal(o["depth_obs"], np.concatenate([r.depth for r in ref]))
    # every output pointer NULL in turn: the others are those of the full call
    a, full = _raw(dets, 4)
    assert _call(h, cfg, a, full, 4) == _lib.QSP_OK
    assert full["is_good"][0] == 1 and not any((v == v.dtype.type(-7)).any() for k, v in full.items() if k not in ("is_good", "kept_flip"))
    for k in _OUT:
        _, o = _raw(dets, 4)
        fresh = o[k].copy()
        assert _call(h, cfg, a, o, 4, drop=("out_" + k,)) == _lib.QSP_OK, k
        assert np.array_equal(o[k], fresh), k
        assert all(np.array_equal(o[j], full[j]) for j in _OUT if j != k), k
    # code == NULL: zero codes
    plain = _tiny(code=False)
    a, zero = _raw(plain, 4)
    assert not a["code"].any()
    assert _call(h, cfg, a, zero, 4) == _lib.QSP_OK
    _, o = _raw(plain, 4)
    assert _call(h, cfg, a, o, 4, drop=("code",)) == _lib.QSP_OK
    assert all(np.array_equal(o[j], zero[j]) for j in _OUT)
    assert not np.array_equal(zero["code"], full["code"])


def test_c_abi_refusals_leave_the_outputs_untouched(gpu_decoder):
    """every refusal is QSP_ERR_INVALID before any launch: no output is written"""
    from qsp_slam_amd import _lib
    from qsp_slam_amd.reconstruct.optimizer import _joint_cfg
    opt = _optimizer(gpu_decoder, n_iter=1)
    cfg, h = _joint_cfg(opt), gpu_decoder.handle
    dets = _tiny()
    a, o = _raw(dets, 4)
    fresh = {k: v.copy() for k, v in o.items()}
    i32 = lambda *v: np.array(v, np.int32)
    n_p, n_f, n_b = int(a["pts_off"][1]), int(a["fg_off"][1]), int(a["bg_off"][1])
    cfg32 = _joint_cfg(opt)
    cfg32.code_len = 32
    refusals = dict(
        pts_off_starts_at_1=dict(pts_off=a["pts_off"] + np.int32(1)), fg_off_starts_at_1=dict(fg_off=a["fg_off"] + np.int32(1)),
        bg_off_starts_at_1=dict(bg_off=a["bg_off"] + np.int32(1)),
        pts_off_decreases=dict(pts_off=i32(0, n_p, n_p - 1)), fg_off_decreases=dict(fg_off=i32(0, n_f, n_f - 1)),
        bg_off_decreases=dict(bg_off=i32(0, n_b, n_b - 1)),
        n_flip_0=dict(n_flip=i32(4, 0)), n_flip_negative=dict(n_flip=i32(-1, 4)), n_flip_65=dict(n_flip=i32(65, 4)),
        no_T_cw=dict(drop=("T_cw",)), no_K=dict(drop=("K",)), no_T_wo=dict(drop=("T_wo",)),
        no_pts_off=dict(drop=("pts_off",)), no_fg_off=dict(drop=("fg_off",)), no_bg_off=dict(drop=("bg_off",)),
        no_pts_world=dict(drop=("pts_world",)), no_fg_px=dict(drop=("fg_px",)), no_fg_world=dict(drop=("fg_world",)),
        no_bg_rays=dict(drop=("bg_rays",)), n_det_0=dict(n_det=0), n_det_negative=dict(n_det=-1))
    for name, kw in refusals.items():
        assert _call(h, cfg, a, o, 4, **kw) == _lib.QSP_ERR_INVALID, name
        assert _lib.lib().qsp_last_error(), name
        assert all(np.array_equal(o[k], fresh[k]) for k in o), name
    assert _call(h, cfg32, a, o, 4) == _lib.QSP_ERR_INVALID          # a code_len that is not the decoder's
    assert b"code_len" in _lib.lib().qsp_last_error()
    assert all(np.array_equal(o[k], fresh[k]) for k in o)
    assert _call(h, cfg, a, o, 4) == _lib.QSP_OK                     # and the same structs unbroken are accepted
    assert not any(np.array_equal(o[k], fresh[k]) for k in o)


def test_group_entry_refuses_a_foreign_class_and_indexes_k_by_detection(gpu_decoder, golden_dir):
    """qsp_refine_detections_group: a det_class outside the group is refused like the rest; two classes, every detection through a
    camera of its own == the per-class calls"""
    from qsp_slam_amd import DeepSdfDecoder, _lib
    from qsp_slam_amd.reconstruct.optimizer import OptimizerGroup, _joint_cfg
    tanh = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz"))
    tanh.set_use_tanh(True)
    opts = {3: _optimizer(gpu_decoder, n_iter=2), 8: _optimizer(tanh, n_iter=2)}
    og = OptimizerGroup(opts)
    try:
        dets = [dc.with_intrinsics(d, K) for d, K in zip(synth.make_detections(20, 4, 200, n_fg=48, n_bg=16, n_kf=2), dc.INTRINSICS)]
        dets[1]["found_good_orientation"] = True
        cids = [8, 3, 8, 3]
        a, o = _raw(dets, 4)
        fresh = {k: v.copy() for k, v in o.items()}
        for bad in ([1, 0, 2, 0], [1, 0, 1, -1]):
            assert _call(og.group.handle, _joint_cfg(opts[3]), a, o, 4, det_class=bad) == _lib.QSP_ERR_INVALID
            assert all(np.array_equal(o[k], fresh[k]) for k in o)
        res = og.refine_detections([dict(d, class_id=c) for d, c in zip(dets, cids)], flip_sample_num=4, taps=True)
        for c in (3, 8):
            idx = [i for i, k in enumerate(cids) if k == c]
            ref = opts[c].refine_detections([dets[i] for i in idx], flip_sample_num=4, taps=True)
            for i, r in zip(idx, ref):
                m = res[i]
                assert all(np.array_equal(m[k], r[k]) for k in ("pts", "rays", "depth", "t_cam_obj_init", "losses")), (c, i)
                assert m.kept_flip == r.kept_flip and m.is_good == r.is_good and np.float32(m.loss) == np.float32(r.loss), (c, i)
                if r.is_good:
                    assert np.array_equal(m.t_cam_obj, r.t_cam_obj) and np.array_equal(m.code, r.code), (c, i)
        assert all(res[i].is_good for i in (1, 3))
        _check_against_oracle(opts[3], [dets[1], dets[3]], 4, [res[1], res[3]])
        # the raw group call gives the wrapper's numbers
        assert _call(og.group.handle, _joint_cfg(opts[3]), a, o, 4, det_class=[1, 0, 1, 0]) == _lib.QSP_OK
        assert np.array_equal(o["rays"], np.concatenate([r.rays for r in res]))
        assert np.array_equal(o["losses"], np.concatenate([r.losses for r in res]))
    finally:
        og.close()
        tanh.close()
