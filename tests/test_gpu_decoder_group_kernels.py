"""Decoder groups on every form of the group kernels (csrc/sdf_kernels.hpp, GRP = true): the narrow split-fp16 tiles, 32-point
Jacobian tiles, both wave counts of the Jacobian and screening kernels (selected per process: QSP_JTJ_WAVES, QSP_JTJ_WAVES_T32,
QSP_SCREEN_WAVES, so those run in a child process), and the group range fallback.  The bar is the one of
tests/test_gpu_decoder_group.py: a mixed-class batch equals one batch per class bit for bit.  The batches are large enough
(6 objects x 4 flips x 2 k points: ~800 Jacobian work items over 256 workgroups) that most workgroups take items of several
classes, so the constants are re-staged inside the kernels."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_FLIP = 4


def _members(name):
    """three classes of one shape: the golden decoder, the same with use_tanh, a seeded perturbation of it"""
    from qsp_slam_amd import DeepSdfDecoder
    path = os.path.join(GOLDEN, name)
    z = np.load(path, allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    rng = np.random.default_rng(5)
    st = {k: (z[k] * (1.0 + 0.02 * rng.standard_normal(z[k].shape))).astype(np.float32) for k in z.files if k != "meta"}
    decs = [DeepSdfDecoder.from_npz(path), DeepSdfDecoder.from_npz(path),
            DeepSdfDecoder.from_state_dict(st, latent_in=meta["latent_in"], code_len=meta["latent_size"])]
    decs[1].set_use_tanh(True)
    return decs


def _cfg(code_len):
    from oracle import sdf_oracle as so
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, _joint_cfg
    from tests.test_gpu_sdf import make_cfg
    return _joint_cfg(Optimizer(None, make_cfg(so.JointConfig(n_iter=3), code_len=code_len)))


def _run(target, cfg, objs, cls):
    from qsp_slam_amd.reconstruct.optimizer import RefineBatch, _flip_rotation
    hyp = np.repeat(np.arange(len(objs)), N_FLIP)
    T0 = np.stack([_flip_rotation(o["t_cam_obj"], k, 2 * np.pi / N_FLIP) for o in objs for k in range(N_FLIP)])
    b = RefineBatch(target, cfg, [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs], hyp,
                    obj_class=cls)
    b.set_state(T0, None)
    b.profile(True)
    b.run(0)
    T, code, loss, good = b.get()
    tr = b.trace()
    prof = b.profile(False)
    b.close()
    out = dict(T=T, code=code, loss=loss, good=good, H=tr["H"], b=tr["b"], dx=tr["dx"], n_valid=tr["n_valid"], K=tr["K"])
    return out, prof


def check_mixed_equals_per_class(decs, cfg, seed=77):
    """6 objects of 2 k points, classes interleaved, 4 flips: the group batch against one batch per class; returns the group
    batch's profile"""
    from qsp_slam_amd import DecoderGroup, synth
    objs = synth.make_object_views(seed, 6, 2000, n_fg=200, n_bg=120)
    cls = np.array([i % 3 for i in range(6)], np.int32)
    g = DecoderGroup(decs)
    mixed, prof = _run(g, cfg, objs, cls)
    g.close()
    for c in range(3):
        idx = np.nonzero(cls == c)[0]
        single, _ = _run(decs[c], cfg, [objs[i] for i in idx], None)
        hyps = np.concatenate([np.arange(N_FLIP) + N_FLIP * i for i in idx])
        assert single["good"].all(), c
        for k, v in single.items():
            assert np.array_equal(mixed[k][hyps], v), (c, k)
    return prof


@pytest.mark.parametrize("tile", [64, 32])
def test_narrow_members_mixed_batch_bit_for_bit(tile):
    """4 x 256 / code 32 members on the narrow split-fp16 tiles: k_mlp_fwd_h2<2, true, 8, true>, k_mlp_jtj_h2<2 or 1, 8, true, true>"""
    decs = _members("decoder_4x256_c32.npz")
    try:
        for d in decs:
            d.set_precision("fp16x2")
            d.set_tile_points(tile)
            assert d.narrow_tile
        check_mixed_equals_per_class(decs, _cfg(32))
    finally:
        for d in decs:
            d.close()


def test_full_width_members_32_point_tiles_bit_for_bit():
    """8 x 512 members at 32-point Jacobian tiles (k_mlp_jtj_h2<1, 4, false, true>), screened forward (k_mlp_fwd_h1<4, true>)"""
    decs = _members("decoder_8x512.npz")
    try:
        for d in decs:
            d.set_precision("fp16x2")
            d.set_tile_points(32)
            d.set_render_screening(0.02)
            d.set_screening_min_samples(0)
        check_mixed_equals_per_class(decs, _cfg(64))
    finally:
        for d in decs:
            d.close()


CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_decoder_group_kernels import _members, _cfg, check_mixed_equals_per_class
decs = _members("decoder_8x512.npz")
for tile in (64, 32):
    for d in decs:
        d.set_precision("fp16x2")
        d.set_tile_points(tile)
        d.set_render_screening(0.02)
        d.set_screening_min_samples(0)
    check_mixed_equals_per_class(decs, _cfg(64))
print("ok")
'''


def test_other_wave_counts_bit_for_bit():
    """the wave counts the defaults do not pick: k_mlp_jtj_h2<2, 4, false, true>, <1, 8, false, true>, k_mlp_fwd_h1<8, true>"""
    env = dict(os.environ, QSP_JTJ_WAVES="4", QSP_JTJ_WAVES_T32="8", QSP_SCREEN_WAVES="8")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_group_range_fallback_repeats_the_whole_call_on_f32():
    """one member (not the first) whose activations leave fp16's range: the whole group call is repeated on the f32 pipe for
    every member, counted once in the profile, and gives the bits of the group on the f32 pipe"""
    from qsp_slam_amd import DecoderGroup, DeepSdfDecoder, synth
    from tests.test_gpu_split_precision import _scaled_decoder
    plain = DeepSdfDecoder.from_npz(os.path.join(GOLDEN, "decoder_8x512.npz"))
    hot = _scaled_decoder(GOLDEN, 1, 6e5, rows=list(range(64)))     # weights inside fp16's range, activations beyond it
    decs = [plain, hot]
    try:
        cfg = _cfg(64)
        objs = synth.make_object_views(88, 4, 600, n_fg=128, n_bg=64)
        cls = np.array([0, 1, 0, 1], np.int32)
        for d in decs:
            d.set_precision("fp16x2")
        n0 = plain.range_fallbacks
        g = DecoderGroup(decs)
        split, prof = _run(g, cfg, objs, cls)
        assert prof.range_fallbacks == 1 and plain.range_fallbacks == n0 + 1
        for d in decs:
            d.set_precision("f32")
        exact, prof32 = _run(g, cfg, objs, cls)
        assert prof32.range_fallbacks == 0
        # (the trace of a hypothesis that stopped early is that of its last iteration -- possibly one of the abandoned fp16
        #  attempt: compared where the hypothesis is alive)
        live = exact["good"]
        assert np.array_equal(split["good"], live) and live[np.repeat(cls == 0, N_FLIP)].all()
        for k, v in exact.items():
            if k in ("H", "b", "dx", "n_valid", "K"):
                assert np.array_equal(split[k][live], v[live], equal_nan=True), k
            else:
                assert np.array_equal(split[k], v, equal_nan=True), k
        # without the fallback the call fails
        for d in decs:
            d.set_precision("fp16x2")
            d.set_range_fallback(False)
        from qsp_slam_amd import _lib
        with pytest.raises(_lib.QspError) as e:
            _run(g, cfg, objs, cls)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED
        g.close()
    finally:
        for d in decs:
            d.close()
