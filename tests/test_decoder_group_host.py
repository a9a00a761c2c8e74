"""CPU: the decoder-group API without a device -- its symbols in the header, the ctypes binding and the library, the Python
argument checks of OptimizerGroup, and the group forms (GRP = true) of the decoder kernels in the compiled ISA (present, inside
the spill budget of their single-decoder twin, clean under the MFMA hazard scan)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SYMBOLS = ["qsp_decoder_group_create", "qsp_decoder_group_destroy", "qsp_refine_batch_create_group",
                 "qsp_reconstruct_objects_group", "qsp_estimate_pose_group", "qsp_refine_detections_group"]

# group kernel (last template argument GRP = true) -> its single-decoder twin in tests/test_isa_budget.py's BUDGET
GROUP_KERNELS = {
    "qsp::k_mlp_jtj_h2<2, 4, false, true>": "qsp::k_mlp_jtj_h2<2, 4, false, false>",
    "qsp::k_mlp_jtj_h2<1, 4, false, true>": "qsp::k_mlp_jtj_h2<1, 4, false, false>",
    "qsp::k_mlp_jtj_h2<2, 8, false, true>": "qsp::k_mlp_jtj_h2<2, 8, false, false>",
    "qsp::k_mlp_jtj_h2<1, 8, false, true>": "qsp::k_mlp_jtj_h2<1, 8, false, false>",
    "qsp::k_mlp_jtj_h2<2, 8, true, true>": "qsp::k_mlp_jtj_h2<2, 8, true, false>",
    "qsp::k_mlp_jtj_h2<1, 8, true, true>": "qsp::k_mlp_jtj_h2<1, 8, true, false>",
    "qsp::k_mlp_fwd_h2<2, false, 4, true>": "qsp::k_mlp_fwd_h2<2, false, 4, false>",
    "qsp::k_mlp_fwd_h2<2, true, 8, true>": "qsp::k_mlp_fwd_h2<2, true, 8, false>",
    "qsp::k_mlp_fwd_h1<4, true>": "qsp::k_mlp_fwd_h1<4, false>",
    "qsp::k_mlp_fwd_h1<8, true>": "qsp::k_mlp_fwd_h1<8, false>",
    "qsp::k_mlp_fwd<false, true>": "qsp::k_mlp_fwd<false, false>",
    "qsp::k_mlp_fwd<true, true>": "qsp::k_mlp_fwd<true, false>",
    "qsp::k_mlp_jtj<false, true>": "qsp::k_mlp_jtj<false, false>",
    "qsp::k_mlp_jtj<true, true>": "qsp::k_mlp_jtj<true, false>",
}
# the per-item parameter lookup is a few scalar registers more across the tile: what a group kernel may spill beyond its twin's
# budget (spilled VGPRs, scratch bytes per lane, spilled SGPRs)
SLACK = (8, 32, 4)


def test_group_symbols_are_declared_bound_and_exported():
    from qsp_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "qsp_hip.h")).read()
    for s in GROUP_SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in _lib.SYMBOLS, s
    so = os.path.join(ROOT, "qsp_slam_amd", "libqsp_hip.so")
    assert os.path.isfile(so), "libqsp_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    assert not [s for s in GROUP_SYMBOLS if s not in exported]


class _Opt(object):
    """the attributes of reconstruct.optimizer.Optimizer that OptimizerGroup reads, no decoder"""

    def __init__(self, **kw):
        base = dict(k1=1.0, k2=100.0, k3=0.25, k4=1e4, b1=0.2, b2=0.02, lr=1.0, s_damp=1.0, cut_off=0.01,
                    num_iterations_joint_optim=5, num_depth_samples=50, code_len=64, decoder=None)
        base.update(kw)
        self.__dict__.update(base)


def test_optimizer_group_refuses_unequal_joint_configs():
    from qsp_slam_amd.reconstruct.optimizer import OptimizerGroup
    with pytest.raises(ValueError, match="joint config"):
        OptimizerGroup({0: _Opt(), 3: _Opt(k2=50.0)})
    with pytest.raises(ValueError, match="joint config"):
        OptimizerGroup({0: _Opt(), 1: _Opt(num_iterations_joint_optim=6)})
    with pytest.raises(ValueError):
        OptimizerGroup({})


def test_optimizer_group_needs_a_class_id_per_object(monkeypatch):
    from qsp_slam_amd import decoder
    from qsp_slam_amd.reconstruct.optimizer import OptimizerGroup

    class NoDeviceGroup(object):
        def __init__(self, decoders):
            self.decoders = decoders
    monkeypatch.setattr(decoder, "DecoderGroup", NoDeviceGroup)
    og = OptimizerGroup({7: _Opt(), 2: _Opt()})
    assert og.class_ids == [2, 7]
    obj = dict(t_cam_obj=None, pts=None, rays=None, depth=None)
    with pytest.raises(ValueError, match="class_id"):
        og.reconstruct_objects_batched([dict(obj, class_id=2), obj])
    with pytest.raises(ValueError, match="class_id"):
        og.refine_detections([dict(obj, class_id=5)])
    with pytest.raises(ValueError, match="class_id"):
        og.estimate_pose_cam_obj([dict(obj)])


def test_group_kernels_are_in_the_isa_inside_their_twins_budget(sdf_isa):
    from tests.test_isa_budget import BUDGET, kernel_metadata
    meta = kernel_metadata(sdf_isa)
    missing = [k for k in GROUP_KERNELS if k not in meta]
    assert not missing, missing
    over = {}
    for k, twin in GROUP_KERNELS.items():
        b = BUDGET[twin]
        m = meta[k]
        if m["vspill"] > b[0] + SLACK[0] or m["scratch"] > b[1] + SLACK[1] or m["sspill"] > b[2] + SLACK[2]:
            over[k] = (m["vspill"], m["scratch"], m["sspill"])
    assert not over, "over budget (spilled VGPRs, scratch bytes per lane, spilled SGPRs): %r" % over


def test_group_kernels_pass_the_mfma_hazard_scan(sdf_isa):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_mfma_hazards as chk
    from tests.test_isa_budget import kernel_metadata
    assert not [k for k in GROUP_KERNELS if k not in kernel_metadata(sdf_isa)]
    n, bad = chk.check(sdf_isa)
    assert not bad, bad[:5]
    assert not chk.check_valu_def_before_mfma(sdf_isa)
