"""GPU: qsp_search_by_projection_kf (the relocalisation and Sim3 projection searches with the result of the reference's serial loop)
against tests/search_projection_kf_oracle.py.

EVERY output of EVERY source and slot must equal the serial restatement: 0 differing, no tolerance (floats compared by bits).  Zero is
derived, not measured: the outputs are integers, plus float32 taps produced by the same IEEE operations in the same order with
contraction off; tests/test_oracle_search_projection_kf.py holds the conditions on the fixtures under which the one operation that
may differ, logf, cannot change a level.  n_rounds must equal the numpy version of the rounds; the chain needs 6.  A run with
QSP_MARGINS_OUT lists the counts under `search_projection_kf/` (the committed copy: profiles/search_projection_kf_margins.json)."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import search_projection_kf_oracle as ko

pytestmark = pytest.mark.gpu

MODES = ko.MODES
IDS = ["reloc", "sim3"]
ALL = [(m, name) for m in MODES for name in ko.fixtures(m)]


def run(f, **over):
    from qsp_slam_amd.ba import search_by_projection_kf
    o = dict(f["opt"], **over)
    return search_by_projection_kf(f["frame"], f["src"], o["mode"], o["th"], orb_dist=o["orb_dist"], check_orientation=o["check_orientation"])


@pytest.fixture(scope="module")
def full():
    return {(m, name): run(ko.fixtures(m)[name]) for m, name in ALL}


@pytest.mark.parametrize("mode,name", ALL, ids=["%s-%s" % (ko.MODE_NAME[m], n) for m, n in ALL])
def test_every_output_equals_the_serial_loop(full, mode, name):
    """contention: two or more sources wanting one key point, the histogram removals; chain: five sources each displacing the next (6
    rounds); edges: ties, the exact thresholds of both modes, the octave windows, NaN and +-0 (RELOC at ORBdist 100 and 64; SIM3 under
    Sim3 scales 0.5 and 2); random: rotated poses, three pyramids and grids, slots taken at entry; stride: frames of 0, 1, 63, 64, 65,
    4096 and 4097 key points"""
    g, r = full[(mode, name)], ko.result(mode, name)
    n = ko.n_differing(g, r)
    print("%s %s: %d sources, %d key points, %d matches, %d rounds: %d outputs differ" % (ko.MODE_NAME[mode], name, len(r["choice"]),
                                                                                       len(r["slot_src"]), r["n_matches"], g["n_rounds"], n))
    assert margins.within("search_projection_kf/%s/%s/outputs_differing" % (ko.MODE_NAME[mode], name), n, 0)
    assert g["n_rounds"] == ko.result_rounds(mode, name)["n_rounds"]
    if name in ("chain", "contention", "contention_no_ori"):
        assert g["n_rounds"] == 6
    if name == "stride_0":
        assert g["n_rounds"] == 1


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_the_named_cases_come_out_as_constructed(full, mode):
    for name in ("contention", "chain", "edges") + (("edges_64", "contention_no_ori") if mode == ko.RELOC else ("scale_half", "scale_two")):
        f, g = ko.fixtures(mode)[name], full[(mode, name)]
        for case, c in f["cases"].items():
            for key in ("choice", "reason", "dist", "bin", "level"):
                if key in c:
                    assert [int(g[key][i]) for i in c["src"]] == list(c[key]), (name, case, key)
            for slot, who in c.get("slot_src", {}).items():
                assert g["slot_src"][slot] == who, (name, case)
        taken = g["choice"][g["choice"] >= 0]
        assert len(set(taken.tolist())) == len(taken) and g["n_matches"] == len(taken) - int((g["slot_src"] == -2).sum()), name


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_source_counts_at_the_launch_edges(mode):
    """1, 3, 4 and 5 sources (four waves per workgroup of the round kernel) of the contention scene and 255, 256 and 257 (the gate
    kernel's lanes) of the random scene repeated: each against the serial loop over that prefix"""
    f = ko.fixtures(mode)["contention"]
    for k in (1, 3, 4, 5):
        cut = dict(f, src=ko.take_sources(f["src"], np.arange(k)))
        assert ko.n_differing(run(cut), ko.serial(cut["frame"], cut["src"], cut["opt"])) == 0, k
    f = ko.fixtures(mode)["random_0"]
    ns = len(f["src"]["valid"])
    for k in (255, 256, 257):
        cut = dict(f, src=ko.take_sources(f["src"], np.arange(k) % ns))          # the pool again: the copies find their slots taken
        g, r = run(cut), ko.serial(cut["frame"], cut["src"], cut["opt"])
        assert ko.n_differing(g, r) == 0 and g["n_rounds"] == ko.rounds(cut["frame"], cut["src"], cut["opt"])["n_rounds"], k


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_the_same_call_twice_has_the_same_bits(full, mode):
    for name in ("contention", "random_0", "stride_4097"):
        g = run(ko.fixtures(mode)[name])
        assert ko.n_differing(g, full[(mode, name)]) == 0 and g["n_rounds"] == full[(mode, name)]["n_rounds"], name


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_unrelated_gated_out_sources_woven_in_change_nothing(full, mode):
    for name in ("contention_no_ori" if mode == ko.RELOC else "contention", "random_1"):
        f = ko.fixtures(mode)[name]
        woven, at = ko.weave(f)
        g, base = run(woven), full[(mode, name)]
        assert (np.delete(g["choice"], at) == -1).all()
        assert not ko.differs({k: np.asarray(v)[at] for k, v in g.items() if k in ko.PER_SOURCE}, base).any(), name
        back = np.full(len(g["choice"]), -9, np.int64)
        back[at] = np.arange(len(at))
        slot = np.asarray(g["slot_src"], np.int64)
        assert np.array_equal(np.where(slot >= 0, back[np.maximum(slot, 0)], slot), base["slot_src"]), name
        assert g["n_matches"] == base["n_matches"] and g["n_rounds"] == base["n_rounds"]
        assert np.array_equal(g["hist"], base["hist"]) and np.array_equal(g["ind"], base["ind"])


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_refusals_leave_the_outputs_untouched(full, mode):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _PROJ_KF_OUT, _PROJ_PTR, _proj_kf_in
    L = _lib.lib()
    f = ko.fixtures(mode)["contention"]
    o = f["opt"]
    i, keep = _proj_kf_in(f["frame"], f["src"], mode, o["th"], o["orb_dist"], o["check_orientation"])
    frame = keep[-2]
    ns, n = int(i.n_src), int(frame.n)
    bufs = {k: np.full(max(ns, n) + 1, 77, dt) for k, dt in _PROJ_KF_OUT + (("slot_src", np.int32),)}
    INV, OK = _lib.QSP_ERR_INVALID, _lib.QSP_OK

    def out(drop=None):
        s = _lib.SearchProjKfOut()
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
        rc = L.qsp_search_by_projection_kf(0, C.byref(inp if inp is not None else i), C.byref(s))
        return rc, s

    def with_(**fields):
        j = _lib.SearchProjKfIn.from_buffer_copy(i)
        for k, v in fields.items():
            setattr(j, k, v)
        return j

    def frame_with(**fields):
        fr = _lib.OrbFrame.from_buffer_copy(frame)
        for k, v in fields.items():
            setattr(fr, k, v)
        keep.append(fr)
        return with_(frame=C.pointer(fr))

    required = ["frame", "slot_blocked", "src_valid", "Xw", "desc", "dist_min_inv", "dist_max_inv", "dist_max"]
    required += ["kp_angle", "src_angle"] if mode == ko.RELOC else ["normal"]
    for name in required:
        rc, s = call(with_(**{name: None}))
        assert rc == INV and untouched(s), name
    for name in ("choice", "dist", "slot_src"):
        rc, s = call(drop=name)
        assert rc == INV and untouched(s), name
    for inp in (with_(n_src=-1), with_(n_src=(1 << 26) + 1), with_(mode=2), with_(mode=3), with_(mode=-1)):
        rc, s = call(inp)
        assert rc == INV and untouched(s)
    if mode == ko.SIM3:
        for inp in (with_(orb_dist=100), with_(orb_dist=49), with_(check_orientation=1)):
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
    assert L.qsp_search_by_projection_kf(0, None, None) == INV
    rc, s = call(with_(n_src=0))                                   # the empty call touches nothing, whatever else it is given
    assert rc == OK and untouched(s)
    assert L.qsp_search_by_projection_kf(0, C.byref(with_(n_src=0, frame=None)), None) == OK
    # every tap NULL: the same required outputs
    s = out()
    taps = ("reason", "level", "proj_x", "proj_y", "bin")
    for k in taps:
        setattr(s, k, None)
    assert L.qsp_search_by_projection_kf(0, C.byref(i), C.byref(s)) == OK
    want = full[(mode, "contention")]
    assert np.array_equal(bufs["choice"][:ns], want["choice"]) and np.array_equal(bufs["slot_src"][:n], want["slot_src"]) and s.n_matches == want["n_matches"]
    assert all((bufs[k] == 77).all() for k in taps)
    assert bufs["choice"][ns] == 77 and bufs["slot_src"][n] == 77
