"""The skip connection's gradient d y / d [code | xyz] of the latent_in layer on the split-fp16 tile (csrc/sdf_mlp.hpp:
mlp_tile_h2<BWD = true>).  The full-width form takes it from layer 4's own backward product -- units 445..511 of that write-out go
to the stash, one padding word into the row -- and the narrow form from a side product; layer 0's backward adds it to the input
gradient.  One Gauss-Newton iteration against oracle/sdf_oracle.py:gn_iteration at north_star's 1e-4 on H and b (the bar of the
teacher-forced and one-iteration tests of tests/test_gpu_sdf.py and tests/test_gpu_narrow.py), block by block, K and n_valid exact:
one hypothesis with 1, 31, 33, 64 and 65 surface points and 16 rays (an empty second point block, a partial one, a second tile), on
f32, bf16x3 and fp16x2 with 64- and 32-point tiles, on a decoder group, and on the narrow 4 x 256 / code 32 decoder.  The four- and
eight-wave kernels are chosen once per process (QSP_JTJ_WAVES, QSP_JTJ_WAVES_T32: tests/test_gpu_jtj_waves.py), so every case runs
in two child processes, started once for the module; the two must agree bit for bit.

The CPU test keeps the others from passing vacuously: the oracle's H with the skip term left out differs from the true H by more
than 100 bars on every one of these inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import sdf_oracle as so
from tests.margins import within
from tests.test_oracle_sdf import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
SIZES = (1, 31, 33, 64, 65)
N_FG, N_BG = 11, 5
FORMS = (("f32", 64), ("bf16x3", 64), ("fp16x2", 64), ("fp16x2", 32))
NARROW_SIZES = (33, 65)
NARROW_FORMS = (("fp16x2", 64), ("fp16x2", 32))
GROUP_SIZE = 65


def full_case(m):
    """one object with m surface points and 16 rays, a non-zero code: inputs of one iteration on the 8 x 512 decoder"""
    from qsp_slam_amd import synth
    o = synth.make_object_views(7000 + m, 1, m, n_fg=N_FG, n_bg=N_BG)[0]
    code = (0.05 * np.random.default_rng(m).standard_normal(64)).astype(np.float32)
    return dict(L=64, t_cam_obj=o["t_cam_obj"], code=code, pts=o["pts"], rays=o["rays"], depth=o["depth"], cfg=so.JointConfig())


def narrow_case(m):
    """the first m surface points of the small decoder's reference fixture, its rays and its first state"""
    from tests.test_oracle_sdf import cfg_from
    j = np.load(os.path.join(GOLDEN, "sdf_small_joint_m400.npz"))
    cfg = cfg_from(j)
    cfg.code_len = 32
    T_co = np.linalg.inv(j["it_T_oc"][0].astype(np.float64)).astype(np.float32)
    return dict(L=32, t_cam_obj=T_co, code=j["it_code"][0].astype(np.float32), pts=j["pts"][:m], rays=j["rays"], depth=j["depth"], cfg=cfg)


def oracle_iteration(odec, c):
    T_oc = np.linalg.inv(c["t_cam_obj"].astype(np.float64)).astype(np.float32)
    n_fg = c["depth"].shape[0]
    dobs = np.concatenate([c["depth"], np.zeros(c["rays"].shape[0] - n_fg, np.float32)])
    return so.gn_iteration(odec, c["cfg"], T_oc, c["code"], c["pts"], c["rays"], dobs, n_fg)


@pytest.fixture(scope="module")
def oracle_runs(oracle_decoder):
    """name -> (case, oracle decoder, the oracle's iteration): computed once, shared, left unchanged"""
    small = so.load_decoder_npz(os.path.join(GOLDEN, "decoder_4x256_c32.npz"))
    runs = {}
    for m in SIZES:
        c = full_case(m)
        runs["full_m%d" % m] = (c, oracle_decoder, oracle_iteration(oracle_decoder, c))
    for m in NARROW_SIZES:
        c = narrow_case(m)
        runs["narrow_m%d" % m] = (c, small, oracle_iteration(small, c))
    return runs


def value_and_grad_without_skip(dec, inp):
    """oracle/sdf_oracle.py:decoder_value_and_input_grad with the latent_in layer's pass-through term g[:, k:] left out"""
    y, masks = so.decoder_forward(dec, inp, keep=True)
    assert not getattr(dec, "use_tanh", False)
    g = ((1 - y * y)[:, None] * dec.layers[-1][0][0][None, :]).astype(np.float32)
    for l in range(len(dec.layers) - 2, -1, -1):
        g = (g * masks[l]) @ dec.layers[l][0]
        if l in dec.latent_in:
            g = g[:, :dec.layers[l][0].shape[1] - inp.shape[1]]
    return y, g.astype(np.float32)


def test_without_the_skip_term_the_oracles_H_is_off_by_more_than_100_bars(oracle_runs, monkeypatch):
    true_H = {name: it["H"] for name, (c, odec, it) in oracle_runs.items()}
    monkeypatch.setattr(so, "decoder_value_and_input_grad", value_and_grad_without_skip)
    for name, (c, odec, it) in oracle_runs.items():
        assert it["fail"] is None and it["K"] >= 1, name
        assert len(odec.latent_in) == 1, name
        n = 7 + c["L"]
        bad = oracle_iteration(odec, c)
        assert bad["K"] == it["K"]                 # (the same rows: only their gradients differ)
        fig = dict(H=relerr(bad["H"], true_H[name]), pose=relerr(bad["H"][:7, :7], true_H[name][:7, :7]),
                   code=relerr(bad["H"][7:n, 7:n], true_H[name][7:n, 7:n]))
        print("skip_gradient/%s: H without the skip term differs by %s" % (name, " ".join("%s %.3g" % kv for kv in fig.items())))
        assert min(fig.values()) >= 100 * BAR, (name, fig)


# ---- the GPU side: every case in one child process per wave count -------------------------------------------------------------

def _iterate(target, joint_cfg, c, obj_class=None):
    from qsp_slam_amd.reconstruct.optimizer import RefineBatch
    b = RefineBatch(target, joint_cfg, [c["pts"]], [c["rays"]], [c["depth"]], [0], obj_class=obj_class)
    b.set_state(c["t_cam_obj"][None], c["code"][None])
    b.run(1)
    tr = b.trace()
    good = b.get()[3]
    b.close()
    return dict(H=tr["H"][0], b=tr["b"][0], K=tr["K"][0], n_valid=tr["n_valid"][0], good=good[0])


def child(out_path):
    """(child process) every case on every form, to one .npz"""
    from qsp_slam_amd import DecoderGroup, DeepSdfDecoder
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, _joint_cfg
    from tests.test_gpu_sdf import make_cfg
    out = {}

    def put(tag, res):
        for k, v in res.items():
            out[tag + "/" + k] = np.asarray(v)
    big = DeepSdfDecoder.from_npz(os.path.join(GOLDEN, "decoder_8x512.npz"))
    twin = DeepSdfDecoder.from_npz(os.path.join(GOLDEN, "decoder_8x512.npz"))
    small = DeepSdfDecoder.from_npz(os.path.join(GOLDEN, "decoder_4x256_c32.npz"))
    assert small.narrow_tile and not big.narrow_tile
    for prec, tile in FORMS:
        for d in (big, twin):
            d.set_precision(prec)
            d.set_tile_points(tile)
        for m in SIZES:
            c = full_case(m)
            put("full_m%d/%s_t%d" % (m, prec, tile), _iterate(big, _joint_cfg(Optimizer(big, make_cfg(c["cfg"]))), c))
        c = full_case(GROUP_SIZE)            # the same object as class 1 of a group of two decoders
        g = DecoderGroup([twin, big])
        try:
            put("group_m%d/%s_t%d" % (GROUP_SIZE, prec, tile),
                _iterate(g, _joint_cfg(Optimizer(None, make_cfg(c["cfg"]))), c, obj_class=np.array([1], np.int32)))
        finally:
            g.close()
    for prec, tile in NARROW_FORMS:
        small.set_precision(prec)
        small.set_tile_points(tile)
        for m in NARROW_SIZES:
            c = narrow_case(m)
            put("narrow_m%d/%s_t%d" % (m, prec, tile), _iterate(small, _joint_cfg(Optimizer(small, make_cfg(c["cfg"], code_len=32))), c))
    assert big.range_fallbacks == 0 and small.range_fallbacks == 0          # the split-fp16 forms are the ones that ran
    for d in (big, twin, small):
        d.close()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def by_waves(tmp_path_factory):
    res = {}
    for waves in ("4", "8"):
        path = str(tmp_path_factory.mktemp("skip_gradient") / ("w%s.npz" % waves))
        env = dict(os.environ, QSP_JTJ_WAVES=waves, QSP_JTJ_WAVES_T32=waves)
        code = "import sys; sys.path.insert(0, sys.argv[1]); from tests.test_gpu_skip_gradient import child; child(sys.argv[2])"
        subprocess.run([sys.executable, "-c", code, ROOT, path], check=True, env=env, timeout=300)
        with np.load(path) as z:
            res[waves] = {k: z[k] for k in z.files}
    return res


def check(by_waves, oracle_runs, tag, oracle_name):
    c, _, it = oracle_runs[oracle_name]
    n = 7 + c["L"]
    assert it["fail"] is None
    for waves in ("4", "8"):
        r = {k: by_waves[waves][tag + "/" + k] for k in ("H", "b", "K", "n_valid", "good")}
        H, b = r["H"][:n, :n], r["b"][:n]
        fig = dict(H=relerr(H, it["H"]), H_pose=relerr(H[:7, :7], it["H"][:7, :7]), H_code=relerr(H[7:, 7:], it["H"][7:, 7:]),
                   H_cross=relerr(H[:7, 7:], it["H"][:7, 7:]), b=relerr(b, it["b"]), b_pose=relerr(b[:7], it["b"][:7]),
                   b_code=relerr(b[7:], it["b"][7:]))
        print("skip_gradient/%s waves %s: K %d (oracle %d) %s" % (tag, waves, int(r["K"]), it["K"],
                                                                   " ".join("%s %.3g" % kv for kv in fig.items())))
        assert bool(r["good"]) and int(r["K"]) == it["K"] and int(r["n_valid"]) == it["n_valid"]
        assert all([within("skip_gradient/%s/%s" % (tag, k), v, BAR) for k, v in fig.items()]), fig


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tile", FORMS, ids=["%s-t%d" % f for f in FORMS])
@pytest.mark.parametrize("m", SIZES)
def test_one_iteration_vs_the_oracle(by_waves, oracle_runs, m, prec, tile):
    check(by_waves, oracle_runs, "full_m%d/%s_t%d" % (m, prec, tile), "full_m%d" % m)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tile", FORMS, ids=["%s-t%d" % f for f in FORMS])
def test_one_iteration_on_a_decoder_group(by_waves, oracle_runs, prec, tile):
    tag = "group_m%d/%s_t%d" % (GROUP_SIZE, prec, tile)
    check(by_waves, oracle_runs, tag, "full_m%d" % GROUP_SIZE)
    for waves in ("4", "8"):         # the group kernel computes what the single-decoder kernel computes
        for k in ("H", "b", "K", "n_valid"):
            assert np.array_equal(by_waves[waves][tag + "/" + k], by_waves[waves]["full_m%d/%s_t%d/%s" % (GROUP_SIZE, prec, tile, k)]), k


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tile", NARROW_FORMS, ids=["%s-t%d" % f for f in NARROW_FORMS])
@pytest.mark.parametrize("m", NARROW_SIZES)
def test_one_iteration_on_the_narrow_decoder(by_waves, oracle_runs, m, prec, tile):
    check(by_waves, oracle_runs, "narrow_m%d/%s_t%d" % (m, prec, tile), "narrow_m%d" % m)


@pytest.mark.gpu
def test_four_and_eight_waves_give_the_same_bits(by_waves):
    assert sorted(by_waves["4"]) == sorted(by_waves["8"]) and len(by_waves["4"]) >= 5 * (len(SIZES) + 1) * len(FORMS)
    for k in by_waves["4"]:
        assert np.array_equal(by_waves["4"][k], by_waves["8"][k], equal_nan=True), k
