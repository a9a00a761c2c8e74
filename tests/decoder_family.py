"""Cases of tests/test_gpu_decoder_family.py: members of the decoder family csrc/sdf_refine.hip:embed_family accepts, chosen on the
boundaries of the skip tables narrow_tables derives (16-wide slabs, 32-wide column blocks, identity slots, the xyz slab of the
latent_in layer), each with seeded weights, one small object and the float64 oracle's Gauss-Newton iteration on it.

Seeded random weights almost never give a render term (the oracle's render_nan exit, K = 0): the zero level set has to pass
through the samples.  So the output layer's bias is shifted by -median(atanh(sdf)) over the object's own surface points at the
start pose and code (SDF values from the oracle).  Seeds and weight scales below were chosen with the oracle alone, on the CPU,
until every entry has fail None, K >= 100 and n_valid >= 1000 (tests/test_decoder_family_cases.py asserts it) and no threshold
decision on a ray sample (|p| < 1, |sdf| < cut-off; decision_margins) of the float64 iteration lies within 2e-5 of its threshold,
twenty times float32's rounding of those values.

CPU only: numpy, the oracle and the synthetic-scene generator."""
import numpy as np

from oracle import sdf_oracle as so
from qsp_slam_amd import synth

M_PTS, N_FG, N_BG = 130, 64, 32      # three 64-point tiles with a ragged last one; <= 96 * 50 ray samples

# name: (code_len, dims, latent_in, narrow form expected, seed, weight scale)
#   dims as in specs.json: the width of a hidden layer's output INCLUDING the re-concatenated [code | xyz] of a latent_in layer
SHAPES = {
    # widths just below / at / above a 32-block and a 16-slab edge
    "c5_33-97-31_in2": (5, [33, 97, 31], (2,), True, 6, 1.0),
    "c16_64-65-63-32_in3": (16, [64, 65, 63, 32], (3,), True, 5, 1.0),
    # column-block counts (3, 10, 5, 2 / 7) that eight waves do not divide
    "c32_96-320-160-40_in3": (32, [96, 320, 160, 40], (3,), True, 9, 1.0),
    "c16_7x200_in3": (16, [200] * 7, (3,), True, 5, 1.0),
    # 424 columns in front of the latent_in layer: ks_in[4] is the full 28 slabs (xyz slab inside the main product); identity slots
    # 1..3 and 7 (seed_full)
    "c63_490-17-130-65_in1": (63, [490, 17, 130, 65], (1,), True, 28, 1.5),
    # 379 columns in front of it: 24 slabs, then the xyz slab on its own
    "c63_445-17-130-65_in1": (63, [445, 17, 130, 65], (1,), True, 16, 1.0),
    # two hidden layers: slots 0 and 4 only, every other slot an identity
    "c16_80-48_in1": (16, [80, 48], (1,), True, 0, 1.0),
    # no latent_in: narrow, narrow with a code of one, narrow at 0.41 of the full shape's multiply-adds (four identity slots pay
    # for layers that wide), and with a fifth layer 0.56 of them: not narrow
    "c1_48-80_none": (1, [48, 80], (), True, 2, 1.0),
    "c64_128-192-96_none": (64, [128, 192, 96], (), True, 24, 1.0),
    "c64_512-400-512-512_none": (64, [512, 400, 512, 512], (), True, 4, 1.0),
    "c64_512-400-512-512-512_none": (64, [512, 400, 512, 512, 512], (), False, 0, 1.0),
    # eight hidden layers of ragged widths, no identity slot: narrow; narrow by a hair (0.497 of the full shape's multiply-adds:
    # the class boundary of narrow_tables); not narrow (0.55)
    "c64_8xragged_narrow_in4": (64, [250, 130, 260, 190, 70, 255, 129, 33], (4,), True, 6, 1.0),
    "c64_8xragged_in4": (64, [512, 300, 400, 512, 256, 512, 100, 512], (4,), True, 3, 1.0),
    "c64_8xragged_wide_in4": (64, [512, 300, 400, 512, 256, 512, 200, 512], (4,), False, 2, 1.0),
}
MIXED = ("c16_64-65-63-32_in3", "c16_7x200_in3", "c16_80-48_in1")      # equal code length, all narrow: one DecoderGroup
ROWS = (("c32_96-320-160-40_in3", "fp16x2"), ("c63_490-17-130-65_in1", "fp16x2"), ("c1_48-80_none", "fp16x2"),
        ("c64_8xragged_wide_in4", "f32"))
POSE_ONLY = ("c5_33-97-31_in2", "c64_128-192-96_none", "c32_96-320-160-40_in3")


def family_layers(rng, L, dims, latent_in, w_scale=1.0):
    """[(W (out, in), None, b (out,))] of deep_sdf/deep_sdf_decoder.py:29-63 for `dims`, seeded normal weights of std w_scale / sqrt(in)"""
    full = [L + 3] + list(dims) + [1]
    layers = []
    for l in range(len(full) - 1):
        out = full[l + 1] - (full[0] if (l + 1) in latent_in else 0)
        w = (w_scale * rng.normal(size=(out, full[l])) / np.sqrt(full[l])).astype(np.float32)
        layers.append((w, None, (0.1 * rng.normal(size=out)).astype(np.float32)))
    return layers


def build_case(name, with_oracle=True):
    """dict(name, L, dims, latent_in, narrow, layers, odec, obj, code, T0 (1,4,4), dobs, cfg[, it: the float64 iteration])"""
    L, dims, latent_in, narrow, seed, w_scale = SHAPES[name]
    rng = np.random.default_rng(1000 + seed)
    layers = family_layers(rng, L, dims, latent_in, w_scale)
    obj = synth.make_object_views(500 + seed, 1, M_PTS, n_fg=N_FG, n_bg=N_BG)[0]
    code = (0.1 * rng.normal(size=L)).astype(np.float32)
    T_oc = np.linalg.inv(obj["t_cam_obj"].astype(np.float64))
    odec = so.DecoderWeights([(w, b) for w, _, b in layers], latent_in, L)
    # the zero level set through the object's own surface points
    y = so.decode_sdf(odec, code, so.transform_points(T_oc.astype(np.float32), obj["pts"]))
    shift = np.float32(np.median(np.arctanh(np.clip(y.astype(np.float64), -0.999999, 0.999999))))
    w_out, _, b_out = layers[-1]
    layers[-1] = (w_out, None, (b_out - shift).astype(np.float32))
    odec = so.DecoderWeights([(w, b) for w, _, b in layers], latent_in, L)
    case = dict(name=name, L=L, dims=dims, latent_in=latent_in, narrow=narrow, layers=layers, odec=odec, obj=obj, code=code,
                T0=obj["t_cam_obj"][None], T_oc=T_oc, dobs=np.concatenate([obj["depth"], np.zeros(N_BG, np.float32)]),
                cfg=so.JointConfig(code_len=L))
    if with_oracle:
        case["it"] = oracle_iteration(case)
    return case


def oracle_iteration(case, f64=True):
    o = case["obj"]
    if f64:
        return so.gn_iteration_f64(case["odec"], case["cfg"], case["T_oc"], case["code"], o["pts"], o["rays"], case["dobs"], N_FG)
    return so.gn_iteration(case["odec"], case["cfg"], case["T_oc"].astype(np.float32), case["code"], o["pts"], o["rays"],
                           case["dobs"], N_FG)


def decision_margins(case):
    """how far the float64 iteration's threshold decisions are from their thresholds: (| |p| - 1 |, | |sdf| - cut-off |) minima
    over the ray samples -- seeds are chosen so that float32 rounding (1e-6) cannot move one across"""
    cfg, o = case["cfg"], case["obj"]
    with so.working_precision(np.float64):
        d64 = so.DecoderWeights(case["odec"].layers, case["latent_in"], case["L"])
        T_oc = case["T_oc"]
        T_co = np.linalg.inv(T_oc)
        scale = np.linalg.det(T_co[:3, :3]) ** (1.0 / 3.0)
        depths = np.linspace(T_co[2, 3] - scale, T_co[2, 3] + scale, cfg.n_depth)
        p = so.transform_points(T_oc, o["rays"].astype(np.float64)[:, None, :] * depths[:, None])
        r = np.sqrt((p * p).sum(-1))
        s = so.decode_sdf(d64, case["code"].astype(np.float64), p[r < 1.0])
    return float(np.abs(r - 1.0).min()), float(np.abs(np.abs(s) - cfg.cut_off).min())
