"""Decoder groups (include/qsp_hip.h, "Decoder groups"): the objects of several classes refined in ONE batch, each work item of
the decoder kernels reading the parameters of its object's class.  The bar is bit identity with one batch per class holding
that class's objects -- on every pipe, screened or not -- plus the reference's own teacher-forced iterations for two classes in
one batch, the detection and pose entry points, the group's resident batch, and every refusal of the group rules."""
import os

import numpy as np
import pytest

from qsp_slam_amd import synth
from tests.test_gpu_sdf import make_cfg
from tests.test_oracle_sdf import relerr

pytestmark = pytest.mark.gpu

N_FLIP = 4
N_PTS = 600          # every object's point count: the slot count nw_sdf (largest point set / 64) is then the same in every batch


def _perturbed(golden_dir, seed=5, eps=0.02):
    """decoder_8x512.npz with every weight and bias multiplied by (1 + eps N(0, 1)), seeded"""
    from qsp_slam_amd import DeepSdfDecoder
    import ast
    z = np.load(os.path.join(golden_dir, "decoder_8x512.npz"), allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    rng = np.random.default_rng(seed)
    st = {k: (z[k] * (1.0 + eps * rng.standard_normal(z[k].shape))).astype(np.float32) for k in z.files if k != "meta"}
    return DeepSdfDecoder.from_state_dict(st, latent_in=meta["latent_in"], code_len=meta["latent_size"])


@pytest.fixture(scope="module")
def members(golden_dir):
    """class 0: decoder_8x512; class 1: the same weights with use_tanh; class 2: perturbed weights"""
    from qsp_slam_amd import DeepSdfDecoder
    path = os.path.join(golden_dir, "decoder_8x512.npz")
    a = DeepSdfDecoder.from_npz(path)
    b = DeepSdfDecoder.from_npz(path)
    b.set_use_tanh(True)
    c = _perturbed(golden_dir)
    yield [a, b, c]
    for d in (a, b, c):
        d.close()


def _set_all(decs, prec, screened=False):
    for d in decs:
        d.set_precision(prec)
        d.set_render_screening(0.02 if screened else 0.0)
        d.set_screening_min_samples(0 if screened else -1)


def _reset(decs):
    _set_all(decs, "f32")


def _redwood(golden_dir):
    return np.load(os.path.join(golden_dir, "sdf_joint_redwood_m600.npz"))


def _objects(golden_dir):
    """the Redwood fixture's observation + synthetic ones, all with N_PTS points"""
    z = _redwood(golden_dir)
    objs = [dict(pts=z["pts"][:N_PTS], rays=z["rays"], depth=z["depth"],
                 t_cam_obj=np.linalg.inv(z["it_T_oc"][0].astype(np.float64)).astype(np.float32))]
    assert objs[0]["pts"].shape[0] == N_PTS
    objs += synth.make_object_views(21, 5, N_PTS, n_fg=200, n_bg=120)
    return objs


def _flip_states(objs):
    from qsp_slam_amd.reconstruct.optimizer import _flip_rotation
    import math
    return np.stack([_flip_rotation(o["t_cam_obj"], k, 2 * math.pi / N_FLIP) for o in objs for k in range(N_FLIP)])


def _run(target, cfg, objs, cls, n_iter):
    from qsp_slam_amd.reconstruct.optimizer import RefineBatch
    hyp = np.repeat(np.arange(len(objs)), N_FLIP)
    b = RefineBatch(target, cfg, [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs], hyp,
                    obj_class=cls)
    b.set_state(_flip_states(objs), None)
    b.run(n_iter)
    out = b.get()
    tr = b.trace()
    prof = b.profile(False)
    b.close()
    return out, tr, prof


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "fp16x2", "fp16x2_screened"])
def test_mixed_batch_equals_single_class_batches_bit_for_bit(members, golden_dir, mode):
    from qsp_slam_amd import DecoderGroup
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, _joint_cfg
    _set_all(members, mode.split("_")[0], mode.endswith("screened"))
    try:
        cfg = _joint_cfg(Optimizer(members[0], make_cfg(_redwood(golden_dir))))
        objs = _objects(golden_dir)
        cls = np.array([i % 3 for i in range(len(objs))], np.int32)       # classes interleaved
        g = DecoderGroup(members)
        (T, code, loss, good), tr, _ = _run(g, cfg, objs, cls, 3)
        g.close()
        for c in range(3):
            idx = np.nonzero(cls == c)[0]
            (Tc, codec, lossc, goodc), trc, _ = _run(members[c], cfg, [objs[i] for i in idx], None, 3)
            hyps = np.concatenate([np.arange(N_FLIP) + N_FLIP * i for i in idx])
            assert np.array_equal(good[hyps], goodc) and goodc.all(), (mode, c)
            for name, mixed, single in (("T", T, Tc), ("code", code, codec), ("loss", loss, lossc)):
                assert np.array_equal(mixed[hyps], single), (mode, c, name)
            for k in ("H", "b", "dx", "n_valid", "K"):
                assert np.array_equal(tr[k][hyps], trc[k]), (mode, c, k)
        # and the classes are different functions: the same object under two decoders does not give the same bits
        assert not np.array_equal(tr["H"][0], _run(members[1], cfg, objs[:1], None, 3)[1]["H"][0])
    finally:
        _reset(members)


@pytest.mark.parametrize("prec", ["f32", "fp16x2"])
def test_two_classes_in_one_batch_meet_the_reference(members, golden_dir, prec):
    """the plain object of sdf_joint_redwood_m600 (class 0) and the use_tanh object of sdf_usetanh_joint_m400 (class 1) in one
    batch, teacher-forced by the reference's iterates: each meets its single-decoder test's bars"""
    from qsp_slam_amd import DecoderGroup
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, RefineBatch, _joint_cfg
    za = _redwood(golden_dir)
    zb = np.load(os.path.join(golden_dir, "sdf_usetanh_joint_m400.npz"))
    _set_all(members, prec)
    try:
        cfg = _joint_cfg(Optimizer(members[0], make_cfg(za)))
        cfg_b = _joint_cfg(Optimizer(members[1], make_cfg(zb)))
        assert [getattr(cfg, f[0]) for f in cfg._fields_] == [getattr(cfg_b, f[0]) for f in cfg._fields_]
        g = DecoderGroup(members[:2])
        b = RefineBatch(g, cfg, [za["pts"], zb["pts"]], [za["rays"], zb["rays"]], [za["depth"], zb["depth"]], [0, 1],
                        obj_class=[0, 1])
        for i in range(min(za["it_H"].shape[0], zb["it_H"].shape[0])):
            T0 = np.stack([np.linalg.inv(z["it_T_oc"][i].astype(np.float64)).astype(np.float32) for z in (za, zb)])
            b.set_state(T0, np.stack([za["it_code"][i], zb["it_code"][i]]))
            b.run(1)
            tr = b.trace()
            for h, z in enumerate((za, zb)):
                assert int(tr["K"][h]) == int(z["it_K"][i]), (prec, h, i)
                assert relerr(tr["H"][h], z["it_H"][i]) < 1e-4, (prec, h, i)
                assert relerr(tr["b"][h], z["it_b"][i]) < 1e-4, (prec, h, i)
        b.close()
        g.close()
    finally:
        _reset(members)


def _det_opt(dec):
    from tests.test_gpu_detections import _optimizer
    return _optimizer(dec, n_iter=3)


def test_refine_detections_by_class_equals_per_class_calls(members):
    """three classes in the group, detections of classes 0 and 2 only, one with n_flip = 1"""
    from qsp_slam_amd.reconstruct.optimizer import OptimizerGroup
    opts = {10 + c: _det_opt(d) for c, d in enumerate(members)}
    dets = synth.make_detections(31, 6, 500, n_fg=96, n_bg=40, n_kf=2)
    dets[3]["found_good_orientation"] = True
    cids = [10, 12, 12, 10, 12, 10]
    for d, c in zip(dets, cids):
        d["class_id"] = c
    og = OptimizerGroup(opts)
    res = og.refine_detections(dets, flip_sample_num=4)
    og.close()
    for c in (10, 12):
        idx = [i for i, k in enumerate(cids) if k == c]
        ref = opts[c].refine_detections([dets[i] for i in idx], flip_sample_num=4)
        for i, r in zip(idx, ref):
            m = res[i]
            assert m.kept_flip == r.kept_flip and m.is_good == r.is_good, (c, i)
            assert np.array_equal(m.losses, r.losses), (c, i)
            if r.is_good:
                assert np.array_equal(m.t_cam_obj, r.t_cam_obj) and np.array_equal(m.code, r.code), (c, i)
    assert res[3].losses.shape == (1,)


def test_estimate_pose_by_class_equals_per_class_calls(members, golden_dir):
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, OptimizerGroup
    cfg = make_cfg(_redwood(golden_dir))
    opts = {c: Optimizer(d, cfg) for c, d in enumerate(members)}
    items = []
    rng = np.random.default_rng(3)
    for i, o in enumerate(synth.make_object_views(41, 5, N_PTS)):
        T = o["t_cam_obj"].astype(np.float64)
        s = np.cbrt(np.linalg.det(T[:3, :3]))
        Tse3 = T.copy()
        Tse3[:3, :3] /= s
        items.append(dict(t_co_se3=Tse3.astype(np.float32), scale=float(s), pts=o["pts"], class_id=[2, 0, 1, 0, 2][i],
                          code=(0.02 * rng.standard_normal(64)).astype(np.float32)))
    og = OptimizerGroup(opts)
    out = og.estimate_pose_cam_obj(items)
    og.close()
    for it, T in zip(items, out):
        ref = opts[it["class_id"]].estimate_pose_cam_obj(it["t_co_se3"], it["scale"], it["pts"], it["code"])
        assert np.array_equal(T, ref)


def test_group_one_shot_does_not_depend_on_what_its_batch_held(members, golden_dir):
    """qsp_reconstruct_objects_group with class mixes A, B, A: the two A calls give the same bits"""
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, OptimizerGroup
    cfg = make_cfg(_redwood(golden_dir))
    og = OptimizerGroup({c: Optimizer(d, cfg) for c, d in enumerate(members)})
    objs = synth.make_object_views(51, 3, 400, n_fg=128, n_bg=64)
    A = [dict(o, class_id=c) for o, c in zip(objs, [0, 1, 2])]
    B = [dict(o, class_id=c) for o, c in zip(synth.make_object_views(52, 4, 900, n_fg=256, n_bg=100), [2, 2, 1, 0])]

    def flat(r):
        return [(x.loss, x.is_good, None if x.t_cam_obj is None else x.t_cam_obj.tobytes()) for f in r for x in f]
    r1 = og.reconstruct_objects_batched(A, flip_sample_num=4, select=False)
    og.reconstruct_objects_batched(B, flip_sample_num=4, select=False)
    r3 = og.reconstruct_objects_batched(A, flip_sample_num=4, select=False)
    assert flat(r1) == flat(r3)
    og.close()


def test_group_refusals(members, golden_dir):
    from qsp_slam_amd import DecoderGroup, DeepSdfDecoder, _lib
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, RefineBatch, _joint_cfg
    import ctypes as C
    small = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_4x256_c32.npz"))
    try:
        with pytest.raises(_lib.QspError) as e:          # code_len 32 against 64
            DecoderGroup([members[0], small])
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED and "code_len" in str(e.value)
    finally:
        small.close()
    try:
        members[1].set_precision("fp16x2")
        with pytest.raises(_lib.QspError) as e:
            DecoderGroup(members)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED and "PRECISION" in str(e.value)
        _set_all(members, "fp16x2")
        members[2].set_render_screening(0.02)
        with pytest.raises(_lib.QspError) as e:
            DecoderGroup(members)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED and "SCREENING" in str(e.value)
    finally:
        _reset(members)
    # a member changed after the group was created: refused at the next group call
    g = DecoderGroup(members)
    cfg = _joint_cfg(Optimizer(members[0], make_cfg(_redwood(golden_dir))))
    o = synth.make_object_views(61, 1, 200, n_fg=64, n_bg=32)[0]
    b = RefineBatch(g, cfg, [o["pts"]], [o["rays"]], [o["depth"]], [0], obj_class=[2])
    b.set_state(o["t_cam_obj"][None], None)
    b.run(1)
    try:
        members[2].set_precision("bf16x3")
        with pytest.raises(_lib.QspError) as e:
            b.run(1)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED
    finally:
        _reset(members)
    b.run(1)
    b.close()
    for bad in (-1, 3):
        with pytest.raises(_lib.QspError) as e:
            RefineBatch(g, cfg, [o["pts"]], [o["rays"]], [o["depth"]], [0], obj_class=[bad])
        assert e.value.code == _lib.QSP_ERR_INVALID
    g.close()
    L = _lib.lib()
    for n in (0, 17):
        hs = (C.c_void_p * 17)(*([members[0].handle.value] * 17))
        h = C.c_void_p()
        assert L.qsp_decoder_group_create(C.cast(hs, C.POINTER(C.c_void_p)), n, C.byref(h)) == _lib.QSP_ERR_INVALID
    g16 = DecoderGroup([members[0]] * 16)       # (the same decoder may stand for several classes)
    g16.close()
