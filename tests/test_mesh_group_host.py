"""CPU: mesh extraction over a decoder group without a device -- its two symbols in the header, the ctypes binding and the
library; the group forms of the grid-decode kernels in the compiled ISA (present, inside the spill budget of their single-decoder
twin plus the group slack, the single-decoder forms still there under their names); the argument checks of MeshExtractorGroup."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_GROUP_SYMBOLS = ["qsp_mesh_extractor_create_group", "qsp_mesh_extract_batch_group"]

# group kernel -> its single-decoder twin in tests/test_isa_budget.py's BUDGET (both are shells around one body: grid_decode_body /
# grid_decode_h2_body<.., GRP>, csrc/sdf_kernels.hpp)
GROUP_KERNELS = {
    "qsp::k_group_grid_decode<false>": "qsp::k_grid_decode<false>",
    "qsp::k_group_grid_decode<true>": "qsp::k_grid_decode<true>",
    "qsp::k_group_grid_decode_h2<false>": "qsp::k_grid_decode_h2<false>",
    "qsp::k_group_grid_decode_h2<true>": "qsp::k_grid_decode_h2<true>",
}


def test_mesh_group_symbols_are_declared_bound_and_exported():
    from qsp_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "qsp_hip.h")).read()
    for s in MESH_GROUP_SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in _lib.SYMBOLS, s
    so = os.path.join(ROOT, "qsp_slam_amd", "libqsp_hip.so")
    assert os.path.isfile(so), "libqsp_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if l.strip()}
    assert not [s for s in MESH_GROUP_SYMBOLS if s not in exported]
    L = _lib.lib()
    assert len(L.qsp_mesh_extractor_create_group.argtypes) == 4 and len(L.qsp_mesh_extract_batch_group.argtypes) == 6


def test_group_grid_decode_kernels_are_in_the_isa_inside_their_twins_budget(sdf_isa):
    from tests.test_decoder_group_host import SLACK
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
    # the single-decoder forms keep their names (tests/test_isa_budget.py looks them up) and their own budgets
    for twin in GROUP_KERNELS.values():
        assert twin in meta, twin
        m, b = meta[twin], BUDGET[twin]
        assert m["vspill"] <= b[0] and m["scratch"] <= b[1] and m["sspill"] <= b[2], (twin, m)
    # nothing else of the grid decode is a kernel: the shared bodies are inlined into the eight entry points
    grid = sorted(k for k in meta if "grid_decode" in k)
    assert grid == sorted(list(GROUP_KERNELS) + list(GROUP_KERNELS.values())), grid


class _Ext(object):
    """the attributes of reconstruct.optimizer.MeshExtractor that MeshExtractorGroup reads, no decoder"""

    def __init__(self, **kw):
        base = dict(voxels_dim=13, code_len=64, method="lewiner", decoder=None)
        base.update(kw)
        self.__dict__.update(base)


class _NoDeviceGroup(object):
    def __init__(self, decoders):
        self.decoders = decoders
        self.closed = False

    def close(self):
        self.closed = True


def test_mesh_extractor_group_refuses_unequal_members(monkeypatch):
    from qsp_slam_amd import decoder
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractorGroup
    monkeypatch.setattr(decoder, "DecoderGroup", _NoDeviceGroup)
    with pytest.raises(ValueError):
        MeshExtractorGroup({})
    with pytest.raises(ValueError, match="voxels_dim"):
        MeshExtractorGroup({0: _Ext(), 3: _Ext(voxels_dim=16)})
    with pytest.raises(ValueError, match="code_len"):
        MeshExtractorGroup({0: _Ext(), 1: _Ext(code_len=32)})
    with pytest.raises(ValueError, match="method"):
        MeshExtractorGroup({0: _Ext(), 1: _Ext(), 2: _Ext(method="table")})


def test_mesh_extractor_group_needs_a_known_class_id_per_code(monkeypatch):
    from qsp_slam_amd import decoder
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractorGroup
    monkeypatch.setattr(decoder, "DecoderGroup", _NoDeviceGroup)
    a, b = _Ext(decoder="a"), _Ext(decoder="b")
    mg = MeshExtractorGroup({7: a, 2: b})
    assert mg.class_ids == [2, 7] and mg.group.decoders == ["b", "a"]      # class index = position among the sorted ids
    assert (mg.voxels_dim, mg.code_len, mg.method) == (13, 64, "lewiner")
    codes = np.zeros((2, 64), np.float32)
    with pytest.raises(ValueError, match="class ids"):
        mg.extract_meshes_from_codes(codes, [2])
    with pytest.raises(ValueError, match="class ids"):
        mg.extract_meshes_from_codes(codes, [2, 7, 7])
    with pytest.raises(ValueError, match="class_id"):
        mg.extract_meshes_from_codes(codes, [2, 5])
    with pytest.raises(ValueError, match="class_id"):
        mg.extract_meshes_from_codes(codes, [None, 7])
    group = mg.group
    mg.close()
    assert group.closed                         # a group it built is its own to close ...
    theirs = _NoDeviceGroup([b, a])
    mg = MeshExtractorGroup({7: a, 2: b}, decoder_group=theirs)
    assert mg.group is theirs
    mg.close()
    assert not theirs.closed                    # ... one it was handed is not
