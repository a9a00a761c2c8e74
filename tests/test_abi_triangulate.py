"""CPU: the library exports the two calls of the CreateNewMapPoints batch, the header declares them, the binding lists them and
its structures have the header's layout."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qsp_triangulate_batch", "qsp_create_new_map_points_batch")


def test_the_new_symbols_are_declared_exported_and_bound():
    from qsp_slam_amd import _lib
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qsp_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert hasattr(L, s), "libqsp_hip.so does not export %s" % s
        assert s in _lib.SYMBOLS
        assert getattr(L, s).argtypes is not None
    assert hasattr(__import__("qsp_slam_amd.ba", fromlist=["x"]), "triangulate_batch")
    assert hasattr(__import__("qsp_slam_amd.ba", fromlist=["x"]), "create_new_map_points_batch")


def test_the_structures_have_the_header_layout():
    """4-byte fields first, then six pointers: no padding but the one in front of the first pointer"""
    from qsp_slam_amd import _lib
    F = _lib.TriangulateFrame
    assert F.Rcw.offset == 4 and F.tcw.offset == 40 and F.Ow.offset == 52 and F.fx.offset == 64 and F.mbf.offset == 92
    assert F.xy_un.offset == 96 and F.scale.offset == 136 and C.sizeof(F) == 144
    assert C.sizeof(_lib.TriangulateGeom) == 32 and _lib.TriangulateGeom.ratio_factor.offset == 24
    assert C.sizeof(_lib.TriangulateOut) == 80
