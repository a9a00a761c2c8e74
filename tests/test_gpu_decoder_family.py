"""The fused refinement kernels on the decoder family (csrc/sdf_refine.hip: embed_family, narrow_tables): one Gauss-Newton
iteration and the pose-only entry point against the float64 evaluation of oracle/sdf_oracle.py, for the shapes of
tests/decoder_family.py -- widths that are no multiple of 64 / 32 / 16, column-block counts that eight waves do not divide, code
lengths 1 / 5 / 16 / 32 / 63 / 64, latent_in at layer 1..4 or absent, identity slots up to the backward seed -- on every launch form
the shape's class allows: f32, bf16x3, fp16x2 at 64- and 32-point tiles, the embedded split-fp16 form of a narrow member, the
screened forward of one that is not narrow; the other wave counts in a child process (they are read once per process).

Bars: north_star's 1e-4 on H, b, the two losses and the next state (cond(H) of every case is ~1e2: the oracle's, asserted below
1e3 or else the state is held to the solve's residual); K and n_valid exact, as
tests/test_gpu_split_precision.py::test_discrete_decisions_match_the_oracle_on_a_random_sweep holds them; rows at the bounds of
tests/test_gpu_sdf.py::test_jacobian_rows_of_fused_kernel_vs_reference; narrow against embedded at the 2e-5 of
tests/test_gpu_narrow.py; pose-only at the 2e-4 of test_pose_only_more_iterations_exercises_the_inlier_filter.  Every figure is
printed before it is asserted, and a run with QSP_MARGINS_OUT lists it under `decoder_family/<shape>/<form>/`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import sdf_oracle as so
from tests import decoder_family as fam
from tests.margins import within
from tests.test_gpu_sdf import make_cfg
from tests.test_oracle_sdf import relerr, rows_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forms_of(name):
    narrow = fam.SHAPES[name][3]
    return ("f32", "bf16x3", "fp16x2", "fp16x2_t32", "fp16x2_embedded" if narrow else "fp16x2_screened")


CASES = [(n, f) for n in fam.SHAPES for f in forms_of(n)]
# a case whose H / b error is above 1e-4 because of ReLU knife-edge rows among its 130 points (decided from batch.rows(), never
# for a dropped block): name/form -> bar, at most 4 x the measured value.  None so far.
KNIFE_EDGE_BAR = {}


class Family(object):
    """the cases, one decoder per shape, and the traces of the forms run so far (narrow against embedded needs two)"""

    def __init__(self):
        from qsp_slam_amd import DeepSdfDecoder
        self.cases = {n: fam.build_case(n) for n in fam.SHAPES}
        self.decs = {n: DeepSdfDecoder(c["layers"], latent_in=c["latent_in"], code_len=c["L"]) for n, c in self.cases.items()}
        self.narrow = {n: d.narrow_tile for n, d in self.decs.items()}
        self.done = {}

    def close(self):
        for d in self.decs.values():
            d.close()

    def set_form(self, name, form):
        d = self.decs[name]
        d.set_precision(form.split("_")[0])
        d.set_tile_points(32 if form.endswith("_t32") else 64)
        if self.narrow[name]:
            d.set_narrow_tile(form != "fp16x2_embedded")
        if form == "fp16x2_screened":
            d.set_render_screening(0.02)
            d.set_screening_min_samples(0)
        elif d.precision == "fp16x2":
            d.set_render_screening(0.0)
        return d

    def batch(self, name, form):
        from qsp_slam_amd.reconstruct.optimizer import Optimizer, RefineBatch, _joint_cfg
        c, d = self.cases[name], self.set_form(name, form)
        o = c["obj"]
        opt = Optimizer(d, make_cfg(c["cfg"], code_len=c["L"]))
        return RefineBatch(d, _joint_cfg(opt), [o["pts"]], [o["rays"]], [o["depth"]], [0])

    def iterate(self, name, form):
        """one iteration from the case's state on `form`: (trace, get), memoised"""
        if (name, form) not in self.done:
            c, d = self.cases[name], self.decs[name]
            n_fb, n_sc = d.range_fallbacks, d.screen_fallbacks
            b = self.batch(name, form)
            b.set_state(c["T0"], c["code"][None])
            b.run(1)
            self.done[(name, form)] = (b.trace(), b.get())
            b.close()
            # the form under test is the one that ran: no repeat on the f32 pipe, no one-pass repeat of a screened run
            assert d.range_fallbacks == n_fb and d.screen_fallbacks == n_sc, (name, form)
        return self.done[(name, form)]


@pytest.fixture(scope="module")
def family():
    f = Family()
    yield f
    f.close()


def check_iteration(f, name, form):
    c = f.cases[name]
    it, L = c["it"], c["L"]
    n = 7 + L
    tr, (T, code, loss, good) = f.iterate(name, form)
    H, b, dx = tr["H"][0].astype(np.float64), tr["b"][0].astype(np.float64), tr["dx"][0].astype(np.float64)
    fig = dict(K=int(tr["K"][0]), n_valid=int(tr["n_valid"][0]), H=relerr(H[:n, :n], it["H"]), b=relerr(b[:n], it["b"]),
               loss_sdf=abs(float(tr["loss_sdf"][0]) - it["loss_sdf"]) / it["loss_sdf"],
               loss_render=abs(float(tr["loss_render"][0]) - it["loss_render"]) / it["loss_render"],
               code_next=float(np.abs(code[0] - it["code_new"]).max()),
               T_oc_next=relerr(np.linalg.inv(T[0].astype(np.float64)), it["T_oc_new"]),
               residual=float(np.abs(H[:n, :n] @ dx[:n] - b[:n]).max() / np.abs(b[:n]).max()), cond=float(np.linalg.cond(it["H"])))
    print("decoder_family/%s/%s: oracle K %d n_valid %d; %s" % (name, form, it["K"], it["n_valid"],
                                                                 " ".join("%s %.3g" % kv for kv in fig.items())))
    # no case passes empty
    assert it["fail"] is None and it["K"] >= 100 and it["n_valid"] >= 1000
    assert bool(good[0]) and code.shape == (1, L)
    assert fig["n_valid"] == it["n_valid"] and fig["K"] == it["K"]
    tag = "decoder_family/%s/%s/" % (name, form)
    bar = KNIFE_EDGE_BAR.get(name + "/" + form, 1e-4)
    ok = [within(tag + "H", fig["H"], bar), within(tag + "b", fig["b"], bar),
          within(tag + "loss_sdf_rel", fig["loss_sdf"], 1e-4), within(tag + "loss_render_rel", fig["loss_render"], 1e-4)]
    # the padding unknowns of a shorter code are decoupled, exactly
    if L < 64:
        assert np.array_equal(tr["H"][0][n:, n:], np.eye(64 - L, dtype=np.float32))
        assert not tr["H"][0][:n, n:].any() and not tr["H"][0][n:, :n].any()
        assert not tr["b"][0][n:].any() and not tr["dx"][0][n:].any()
    # the next state: dx = H^-1 b amplifies the error of H, b by cond(H) (the note above TEACHER_FORCED_TOL, tests/test_gpu_sdf.py)
    if fig["cond"] < 1e3:
        ok += [within(tag + "code_next_abs", fig["code_next"], 1e-4), within(tag + "T_oc_next", fig["T_oc_next"], 1e-4)]
    else:
        ok += [within(tag + "solve_residual", fig["residual"], 1e-4)]
    assert all(ok), fig
    if form == "fp16x2_embedded":       # the two forms of the split-fp16 tile on the same decoder
        tn = f.iterate(name, "fp16x2")[0]
        assert int(tn["K"][0]) == fig["K"] and int(tn["n_valid"][0]) == fig["n_valid"]
        assert within(tag + "vs_narrow/H", relerr(tn["H"][0], tr["H"][0]), 2e-5)
        assert within(tag + "vs_narrow/b", relerr(tn["b"][0], tr["b"][0]), 2e-5)


def test_every_shape_is_of_the_class_the_table_expects(family):
    from qsp_slam_amd import _lib
    for name, d in family.decs.items():
        assert family.narrow[name] == fam.SHAPES[name][3], name
        if not family.narrow[name]:
            with pytest.raises(_lib.QspError) as e:
                d.set_narrow_tile(True)
            assert e.value.code == _lib.QSP_ERR_UNSUPPORTED


@pytest.mark.parametrize("name,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_one_iteration_vs_the_float64_oracle(family, name, form):
    check_iteration(family, name, form)


@pytest.mark.parametrize("name,form", fam.ROWS, ids=["%s-%s" % c for c in fam.ROWS])
def test_jacobian_rows_vs_the_float64_oracle(family, name, form):
    """what the fused kernel feeds to the normal equations, row by row: a dropped column block shows here even where H hides it"""
    c = family.cases[name]
    it, L, cfg = c["it"], c["L"], c["cfg"]
    b = family.batch(name, form)
    b.enable_rows(True)
    b.set_state(c["T0"], c["code"][None])
    b.run(1)
    K = int(b.trace()["K"][0])
    assert K == it["K"]
    rs, rr = b.rows(0, fam.M_PTS, K)
    b.close()
    assert rows_close(rs[:, :7], it["Jp_sdf"]) and rows_close(rs[:, 7:7 + L], it["Jc_sdf"])
    assert rows_close(rr[:, :7], it["Jp_render"], tol=2e-5, max_bad=0.02)
    assert rows_close(rr[:, 7:7 + L], it["Jc_render"], tol=2e-5, max_bad=0.02)
    assert not rs[:, 7 + L:71].any() and not rr[:, 7 + L:71].any()
    with so.working_precision(np.float64):
        rob_s, rob_r = so.robust_residual(it["res_sdf"], cfg.b2)[0], so.robust_residual(it["res_render"], cfg.b1)[0]
    assert np.abs(rs[:, 71] - rob_s).max() < 1e-5 * max(np.abs(rob_s).max(), 1e-6) + 1e-7
    assert np.abs(rr[:, 71] - rob_r).max() < 1e-4 * np.abs(rob_r).max()


@pytest.mark.parametrize("prec", ["f32", "fp16x2"])
@pytest.mark.parametrize("name", fam.POSE_ONLY)
def test_pose_only_vs_the_oracle(family, name, prec):
    from qsp_slam_amd.reconstruct.optimizer import Optimizer
    c = family.cases[name]
    d = family.set_form(name, prec)
    T = c["obj"]["t_cam_obj"].astype(np.float64)
    s = np.linalg.det(T[:3, :3]) ** (1 / 3)
    T_se3 = T.copy()
    T_se3[:3, :3] /= s
    ref = so.estimate_pose_cam_obj(c["odec"], c["cfg"], T_se3.astype(np.float32), float(s), c["obj"]["pts"], c["code"])
    out = Optimizer(d, make_cfg(c["cfg"], code_len=c["L"])).estimate_pose_cam_obj(T_se3.astype(np.float32), float(s), c["obj"]["pts"],
                                                                                 c["code"])
    assert relerr(ref, T_se3) > 1e-3                  # the five iterations moved the pose
    assert within("decoder_family/%s/%s/pose_only_t_co" % (name, prec), relerr(out, ref), 2e-4)


def _mixed_batch(target, cfg, cases, names, obj_class):
    """one object per entry of `names` (that case's own, so that its render term exists), two start poses each, one iteration"""
    from qsp_slam_amd.reconstruct.optimizer import RefineBatch
    objs = [cases[n]["obj"] for n in names]
    T0, code = [], []
    for n in names:
        for shift in (0.0, 2e-3):
            T = cases[n]["T0"][0].copy()
            T[0, 3] += np.float32(shift)
            T0.append(T)
            code.append(cases[n]["code"])
    b = RefineBatch(target, cfg, [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                    np.repeat(np.arange(len(objs)), 2), obj_class=obj_class)
    b.set_state(np.stack(T0), np.stack(code))
    b.run(1)
    T, z, loss, good = b.get()
    out = dict(b.trace(), T=T, code=z, loss=loss, good=good)
    b.close()
    return out


@pytest.mark.parametrize("form", ["f32", "fp16x2", "fp16x2_t32"])
def test_members_of_different_shapes_in_one_group_bit_for_bit(family, form):
    """a decoder group takes members of different shapes (group_options asks for equal code length and options, the narrow flag
    among them, not for equal skip tables): the mixed batch equals one batch per class bit for bit"""
    from qsp_slam_amd import DecoderGroup
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, _joint_cfg
    members = fam.MIXED
    decs = [family.set_form(n, form) for n in members]
    cfg = _joint_cfg(Optimizer(None, make_cfg(so.JointConfig(), code_len=family.cases[members[0]]["L"])))
    cls = np.array([0, 1, 2, 0, 1, 2], np.int32)
    g = DecoderGroup(decs)
    try:
        mixed = _mixed_batch(g, cfg, family.cases, [members[c] for c in cls], cls)
    finally:
        g.close()
    assert mixed["good"].all() and (mixed["K"] >= 100).all()
    for c in range(3):
        single = _mixed_batch(decs[c], cfg, family.cases, [members[c]] * 2, None)
        hyps = np.concatenate([[2 * o, 2 * o + 1] for o in np.nonzero(cls == c)[0]])
        for k, v in single.items():
            assert np.array_equal(mixed[k][hyps], v), (members[c], k)


def test_a_group_refuses_members_of_different_code_length_or_class(family):
    from qsp_slam_amd import DecoderGroup, _lib
    a = family.set_form("c16_7x200_in3", "fp16x2")
    for other in ("c32_96-320-160-40_in3",):                      # code 32 against code 16
        with pytest.raises(_lib.QspError) as e:
            DecoderGroup([a, family.set_form(other, "fp16x2")])
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED
    n64, w64 = family.set_form("c64_128-192-96_none", "fp16x2"), family.set_form("c64_8xragged_wide_in4", "fp16x2")
    with pytest.raises(_lib.QspError) as e:                        # equal code length, narrow against not narrow
        DecoderGroup([n64, w64])
    assert e.value.code == _lib.QSP_ERR_UNSUPPORTED


CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_decoder_family as t
f = t.Family()
for name, form in t.CASES:
    if form.startswith("fp16x2"):
        t.check_iteration(f, name, form)
f.close()
print("ok")
'''


def test_other_wave_counts_vs_the_float64_oracle():
    """the wave counts the defaults do not pick (k_mlp_jtj_h2<2, 4, ..>, <1, 8, ..>, k_mlp_fwd_h1<8>): every split-fp16 case again"""
    env = dict(os.environ, QSP_JTJ_WAVES="4", QSP_JTJ_WAVES_T32="8", QSP_SCREEN_WAVES="8")
    env.pop("QSP_MARGINS_OUT", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
