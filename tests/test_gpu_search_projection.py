"""GPU: qsp_search_by_projection (tracking's two projection searches with the result of the reference's serial loop) against
tests/search_projection_oracle.py.

EVERY output of EVERY source and slot must equal the serial restatement: 0 differing, no tolerance (floats compared by bits).
tests/test_oracle_search_projection.py holds the conditions on the fixtures under which that can be asked.  n_rounds must equal the
numpy version of the rounds; the chain needs 6.  A run with QSP_MARGINS_OUT lists the counts under `search_projection/` (the
committed copy: profiles/search_projection_margins.json)."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import search_projection_oracle as po

pytestmark = pytest.mark.gpu

MODES = (po.LOCAL, po.LAST)
MODE_NAME = {po.LOCAL: "local", po.LAST: "last"}
ALL = [(m, name) for m in MODES for name in po.fixtures(m)]


def run(f, **over):
    from qsp_slam_amd.ba import search_by_projection
    o = dict(f["opt"], **over)
    return search_by_projection(f["frame"], f["src"], mode=o["mode"], th=o["th"], nn_ratio=o["nn_ratio"], view_cos_limit=o["view_cos_limit"],
                                check_orientation=o["check_orientation"], mono=o["mono"], last_Rcw=o["last_Rcw"], last_tcw=o["last_tcw"], tap=True)


@pytest.fixture(scope="module")
def full():
    return {(m, name): run(po.fixtures(m)[name]) for m, name in ALL}


def n_differing(g, r, mode, ori):
    """sources with any differing output + slots with a differing holder + differing scalars of the call"""
    n = int(po.differs(g, r, mode, ori).sum()) + int((np.asarray(g["slot_src"], np.int64) != r["slot_src"]).sum()) + int(g["n_matches"] != r["n_matches"])
    if mode == po.LAST:
        n += int((np.asarray(g["hist"], np.int64) != r["hist"]).sum()) + int(list(g["ind"]) != list(r["ind"]))
    return n


@pytest.mark.parametrize("mode,name", ALL, ids=["%s-%s" % (MODE_NAME[m], n) for m, n in ALL])
def test_every_output_equals_the_serial_loop(full, mode, name):
    """contention: every case of two or more sources wanting one key point; chain: five sources each displacing the next (6 rounds);
    edges: ties, stereo and mono key points, levels 0 and top, the exact thresholds, NaN and +-0, under th == 1 and th != 1 (LOCAL)
    and forward, backward, neither and mono (LAST); random: a rotated pose, three pyramids and grids, slots taken at entry; stride:
    frames of 0, 1, 63, 64, 65 and 4097 key points"""
    f, g, r = po.fixtures(mode)[name], full[(mode, name)], po.result(mode, name)
    n = n_differing(g, r, mode, f["opt"]["check_orientation"])
    print("%s %s: %d sources, %d key points, %d matches, %d rounds: %d outputs differ" % (MODE_NAME[mode], name, len(r["choice"]),
                                                                                       len(r["slot_src"]), r["n_matches"], g["n_rounds"], n))
    assert margins.within("search_projection/%s/%s/outputs_differing" % (MODE_NAME[mode], name), n, 0)
    assert g["n_rounds"] == po.result_rounds(mode, name)["n_rounds"]
    if name in ("chain", "contention", "contention_no_ori"):
        assert g["n_rounds"] == 6


@pytest.mark.parametrize("mode", MODES, ids=["local", "last"])
def test_the_named_cases_come_out_as_constructed(full, mode):
    for name in ("contention", "chain", "edges" if mode == po.LOCAL else "edges_neither"):
        f, g = po.fixtures(mode)[name], full[(mode, name)]
        for case, c in f["cases"].items():
            for key in ("choice", "reason", "dist", "dist2", "bin"):
                if key in c:
                    assert [int(g[key][i]) for i in c["src"]] == list(c[key]), (name, case, key)
            for slot, who in c.get("slot_src", {}).items():
                assert g["slot_src"][slot] == who, (name, case)
    if mode == po.LAST:
        c = po.fixtures(mode)["edges_neither"]["cases"]["windows"]
        for d, want in list(c["by_direction"].items()) + [("mono", c["by_direction"]["neither"])]:   # mono: the forward pose, no direction
            assert full[(mode, "edges_" + d)]["choice"][c["src"][0]] == want, d


@pytest.mark.parametrize("mode", MODES, ids=["local", "last"])
def test_source_counts_at_the_workgroup_edges(full, mode):
    """0, 1, 3, 4 and 5 sources (four waves per workgroup): the first k sources of the contention scene, whose serial values do not
    depend on the sources after them"""
    f = po.fixtures(mode)["contention"]
    for k in (0, 1, 3, 4, 5):
        cut = dict(f, src=po.take_sources(f["src"], np.arange(k)))
        g, r = run(cut), po.serial(cut["frame"], cut["src"], cut["opt"])
        if k == 0:
            assert g["n_rounds"] == 0 and g["n_matches"] == 0 and (g["slot_src"] == -1).all() and len(g["choice"]) == 0
            continue
        assert n_differing(g, r, mode, True) == 0, k                 # against the serial loop over the k sources, `bin` included
        # ... and against the first k sources of the full call, without `bin`: the cut keeps a match that the full call's histogram
        # may null (the first boxes hold no orientation case: the histogram tail at full size is the contention scene's own test)
        assert not po.differs(g, {key: np.asarray(v)[:k] for key, v in full[(mode, "contention")].items() if key in po.PER_SOURCE}, mode, False).any(), k


@pytest.mark.parametrize("mode", MODES, ids=["local", "last"])
def test_the_same_call_twice_has_the_same_bits(full, mode):
    for name in ("contention", "random_0", "stride_4097"):
        assert po.same_call(run(po.fixtures(mode)[name]), full[(mode, name)], mode), name


@pytest.mark.parametrize("mode", MODES, ids=["local", "last"])
def test_unrelated_gated_out_sources_woven_in_change_nothing(full, mode):
    for name in ("contention", "random_1"):
        f = po.fixtures(mode)[name]
        woven, at = po.weave(f, mode)
        g, base = run(woven), full[(mode, name)]
        assert (np.delete(g["choice"], at) == -1).all()
        assert not po.differs({k: np.asarray(v)[at] for k, v in g.items() if k in po.PER_SOURCE}, base, mode, True).any(), name
        back = np.full(len(g["choice"]), -9, np.int64)
        back[at] = np.arange(len(at))
        slot = np.asarray(g["slot_src"], np.int64)
        assert np.array_equal(np.where(slot >= 0, back[np.maximum(slot, 0)], slot), base["slot_src"]), name
        assert g["n_matches"] == base["n_matches"] and g["n_rounds"] == base["n_rounds"]


@pytest.mark.parametrize("mode", MODES, ids=["local", "last"])
def test_refusals_leave_the_outputs_untouched(full, mode):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _PROJ_OUT, _PROJ_PTR, _proj_in
    L = _lib.lib()
    f = po.fixtures(mode)["contention"]
    o = f["opt"]
    i, keep = _proj_in(f["frame"], f["src"], mode, o["th"], o["nn_ratio"], o["view_cos_limit"], o["check_orientation"], o["mono"], o["last_Rcw"], o["last_tcw"])
    frame, arrays = keep[-2], keep[-1]
    ns, n = int(i.n_src), int(frame.n)
    bufs = {k: np.full(max(ns, n) + 1, 77, dt) for k, dt in _PROJ_OUT + (("slot_src", np.int32),)}
    INV, OK = _lib.QSP_ERR_INVALID, _lib.QSP_OK

    def out(drop=None):
        s = _lib.SearchProjOut()
        for k, b in bufs.items():
            if k != drop:
                setattr(s, k, _PROJ_PTR[b.dtype.type](b))
        s.n_matches, s.n_rounds = -7, -7
        s.hist[:] = [-7] * 30
        s.ind[:] = [-7] * 3
        return s

    def untouched(s):
        return all((b == 77).all() for b in bufs.values()) and s.n_matches == -7 and s.n_rounds == -7 and list(s.hist) == [-7] * 30 and list(s.ind) == [-7] * 3

    def call(inp=None, drop=None):
        s = out(drop)
        rc = L.qsp_search_by_projection(0, C.byref(inp if inp is not None else i), C.byref(s))
        return rc, s

    def with_(**fields):
        j = _lib.SearchProjIn.from_buffer_copy(i)
        for k, v in fields.items():
            setattr(j, k, v)
        return j

    def frame_with(**fields):
        fr = _lib.OrbFrame.from_buffer_copy(frame)
        for k, v in fields.items():
            setattr(fr, k, v)
        keep.append(fr)
        return with_(frame=C.pointer(fr))

    required = ["frame", "u_right", "slot_blocked", "src_valid", "src_blocks", "Xw", "desc"]
    required += ["normal", "dist_min_inv", "dist_max_inv", "dist_max"] if mode == po.LOCAL else ["src_octave", "src_angle", "kp_angle"]
    for name in required:
        rc, s = call(with_(**{name: None}))
        assert rc == INV and untouched(s), name
    for name in ("choice", "dist", "slot_src") + (("in_view", "proj_x", "proj_y", "proj_xr", "level", "view_cos") if mode == po.LOCAL else ()):
        rc, s = call(drop=name)
        assert rc == INV and untouched(s), name
    for inp in (with_(n_src=-1), with_(n_src=(1 << 26) + 1), with_(mode=2), with_(mode=-1)):
        rc, s = call(inp)
        assert rc == INV and untouched(s)
    octs = np.array(f["frame"]["octave"], np.int32)
    bad_oct, neg_oct = octs.copy(), octs.copy()
    bad_oct[2], neg_oct[2] = len(f["frame"]["scale_factors"]), -1
    keep += [bad_oct, neg_oct]
    for fields in (dict(n=-1), dict(n=(1 << 26) + 1), dict(n_levels=17), dict(n_levels=0), dict(grid_cols=65), dict(grid_rows=0), dict(grid_cols=0),
                   dict(octave=_lib.i32ptr(bad_oct)), dict(octave=_lib.i32ptr(neg_oct)), dict(kp=None), dict(desc=None), dict(octave=None),
                   dict(scale_factors=None)):
        rc, s = call(frame_with(**fields))
        assert rc == INV and untouched(s), fields
    if mode == po.LAST:
        for v in (-1, len(f["frame"]["scale_factors"])):
            so_ = arrays["src_octave"].copy()
            so_[1] = v
            keep.append(so_)
            rc, s = call(with_(src_octave=_lib.i32ptr(so_)))
            assert rc == INV and untouched(s), v
    assert L.qsp_search_by_projection(0, None, None) == INV
    rc, s = call(with_(n_src=0))                                   # the empty call touches nothing, whatever else it is given
    assert rc == OK and untouched(s)
    assert L.qsp_search_by_projection(0, C.byref(with_(n_src=0, frame=None)), None) == OK
    # every tap NULL: the same required outputs
    s = out()
    for k in ("reason", "dist2", "level_best", "level2", "bin"):
        setattr(s, k, None)
    assert L.qsp_search_by_projection(0, C.byref(i), C.byref(s)) == OK
    want = full[(mode, "contention")]
    assert np.array_equal(bufs["choice"][:ns], want["choice"]) and np.array_equal(bufs["slot_src"][:n], want["slot_src"]) and s.n_matches == want["n_matches"]
    assert all((bufs[k] == 77).all() for k in ("reason", "dist2", "level_best", "level2", "bin"))
    assert bufs["choice"][ns] == 77 and bufs["slot_src"][n] == 77
