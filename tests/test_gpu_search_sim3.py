"""GPU: qsp_search_by_sim3_batch (SearchBySim3 for all loop candidates in one call) against tests/search_sim3_oracle.py.

The tap (best1 / best2 / dist1 / dist2: the two passes before the agreement step) must equal the float64 flavour's on every source
slot whose knife-edge distance is at least BAND = 4 x the band measured on the CPU between the oracle's two flavours; match12 and
n_found wherever both slots of the pair are outside the band.  tests/test_oracle_search_sim3.py holds the conditions on the
fixtures under which the band decides next to nothing (at most 2 % of a candidate's source slots).  A candidate's outputs have the
same bits alone, in any batch and at any position.  Every figure is printed before it is asserted; a run with QSP_MARGINS_OUT
lists them under `search_sim3/` (the committed copy: profiles/search_sim3_margins.json)."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import search_sim3_oracle as so

pytestmark = pytest.mark.gpu

KEYS = ("match12", "best1", "dist1", "best2", "dist2")


def run(cands):
    from qsp_slam_amd.ba import search_by_sim3_batch
    return search_by_sim3_batch(so.key_frame_1(), cands, tap=True)


@pytest.fixture(scope="module")
def full():
    return run(so.pool())


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and a["n_found"] == b["n_found"]


def test_both_passes_equal_the_oracle_outside_the_band(full):
    width = so.band()
    margins.within("search_sim3/band_f32_vs_f64", so.measured(), width)
    worst = 0.0
    for i, (r, g) in enumerate(zip(so.pool_results("f64"), full)):
        n_diff = 0
        for d in (1, 2):
            diff = (g["best%d" % d] != r["best%d" % d]) | (g["dist%d" % d] != r["dist%d" % d])
            n_diff += int(diff.sum())
            if diff.any():
                worst = max(worst, float(r["knife%d" % d][diff].max()))
        share = so.in_band_share(r, width)
        print("candidate %2d (n2 = %3d): %d source slots differ from float64, %.4f of the slots inside the band"
              % (i, len(r["best2"]), n_diff, share))
        assert share <= so.IN_BAND_CAP, (i, share)
    print("largest knife-edge distance of a differing slot %.3e, BAND %.3e" % (worst, width))
    # a slot may differ only strictly inside the band: `worst` is 0 when none differs, and then passes a band of 0 as well
    assert margins.within("search_sim3/slot_edge", worst, width) and (worst < width or worst == 0.0)


def test_agreement_equals_the_oracle_outside_the_band(full):
    width = so.band()
    for i, (r, g) in enumerate(zip(so.pool_results("f64"), full)):
        sure = r["knife1"] >= width
        j = r["best1"]
        sure &= np.where(j >= 0, r["knife2"][np.maximum(j, 0)] >= width, True) if len(r["knife2"]) else True
        assert np.array_equal(g["match12"][sure], r["match12"][sure]), i
        assert g["n_found"] == int((g["match12"] >= 0).sum())
        if sure.all():
            assert g["n_found"] == r["n_found"], (i, g["n_found"], r["n_found"])
        assert (g["match12"][np.asarray(so.pool()[i]["pre1"], bool)] == -1).all()


def test_the_named_cases(full):
    sp, g = so.special_candidate(), full[so.I_SPECIAL]
    n = so.NAMED
    for name, first in sp["tie_first"].items():                # ties go to the first in (cell x, cell y, index), not to the lowest index
        assert g["best1"][n[name]] == first and first != sp["tie_lowest"][name], (name, g["best1"][n[name]])
    assert g["dist1"][n["th_100"]] == 100 and g["best1"][n["th_100"]] >= 0          # TH_HIGH is inclusive
    assert g["dist1"][n["th_101"]] == 101 and g["best1"][n["th_101"]] == -1
    assert g["best1"][n["unfiled"]] == sp["unfiled_filed"] and g["dist1"][n["unfiled"]] == 40   # the perfect key point was never filed
    assert g["dist1"][n["octaves"]] == 20
    assert g["best1"][n["no_mutual"]] >= 0 and g["match12"][n["no_mutual"]] == -1
    pb = sp["pre2_best"]
    assert g["best1"][n["pre2_best"]] == pb and g["best2"][pb] == -1 and g["dist2"][pb] == -1 and g["match12"][n["pre2_best"]] == -1
    assert g["best1"][n["empty_box"]] == -1 and g["dist1"][n["empty_box"]] == -1
    assert g["match12"][n["tie_cx"]] == sp["tie_first"]["tie_cx"] and g["n_found"] == 1
    small = full[so.I_SMALL]                                   # the unfiled key point of the small image is nobody's best
    assert (small["best1"] != min(len(small["best2"]), 40) - 1).all()


def test_alone_in_any_batch_at_any_position(full):
    cands = so.pool()
    for i, c in enumerate(cands):                              # batches of 1
        assert same_bits(run([c])[0], full[i]), i
    rev = run(cands[::-1])                                     # every other position
    for r, g in zip(rev[::-1], full):
        assert same_bits(r, g)
    twice = run(cands + cands)                                 # the pool twice in one call
    for k, r in enumerate(twice):
        assert same_bits(r, full[k % len(cands)]), k


def _raw(cands, tap=True):
    """the structs of a call over `cands`, built by hand so that single fields can be broken"""
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _orb_frame
    keep = []
    f1 = _orb_frame(so.key_frame_1(), keep)
    f2 = (_lib.OrbFrame * len(cands))(*[_orb_frame(c["kf2"], keep) for c in cands])
    n1, n2 = f1.n, [f.n for f in f2]
    a = dict(off2=np.concatenate([[0], np.cumsum(n2)]).astype(np.int32),
             K=np.ascontiguousarray(np.stack([c["K"] for c in cands]), np.float32), s12=np.array([c["s12"] for c in cands], np.float32),
             R12=np.ascontiguousarray(np.stack([c["R12"].reshape(9) for c in cands]), np.float32),
             t12=np.ascontiguousarray(np.stack([c["t12"] for c in cands]), np.float32), th=np.array([c["th"] for c in cands], np.float32),
             pre1=np.concatenate([c["pre1"] for c in cands]).astype(np.uint8), pre2=np.concatenate([c["pre2"] for c in cands]).astype(np.uint8))
    o = dict(match12=np.full(len(cands) * n1, -7, np.int32), n_found=np.full(len(cands), -5, np.int32),
             best1=np.full(len(cands) * n1, -3, np.int32), dist1=np.full(len(cands) * n1, -3, np.int32),
             best2=np.full(sum(n2), -3, np.int32), dist2=np.full(sum(n2), -3, np.int32))
    return keep, f1, f2, a, o


def test_error_paths_leave_the_outputs_untouched(full):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import search_by_sim3_batch
    assert search_by_sim3_batch(so.key_frame_1(), []) == []
    L = _lib.lib()
    idx = (4, 2)
    cands = [so.pool()[i] for i in idx]
    keep, f1, f2, a, o = _raw(cands)
    fresh = {k: v.copy() for k, v in o.items()}
    untouched = lambda: all(np.array_equal(o[k], fresh[k]) for k in o)

    def call(n_cand=2, drop_in=None, drop_out=None, tap=True, kf1=None, kf2=None, **kw):
        b = dict(a, **{k: np.ascontiguousarray(v, a[k].dtype) for k, v in kw.items()})
        ptr = {k: (_lib.fptr(v) if v.dtype == np.float32 else _lib.i32ptr(v) if v.dtype == np.int32 else _lib.u8ptr(v)) for k, v in b.items()}
        if drop_in in ptr:
            ptr[drop_in] = None
        i = _lib.SearchSim3In(n_cand, None if drop_in == "kf1" else C.pointer(kf1 or f1), None if drop_in == "kf2" else (kf2 or f2),
                              ptr["off2"], ptr["K"], ptr["s12"], ptr["R12"], ptr["t12"], ptr["th"], ptr["pre1"], ptr["pre2"])
        outs = [None if (k == drop_out or (not tap and k not in ("match12", "n_found"))) else _lib.i32ptr(o[k])
                for k in ("match12", "n_found", "best1", "dist1", "best2", "dist2")]
        out = _lib.SearchSim3Out(*outs)
        return L.qsp_search_by_sim3_batch(0, C.byref(i), C.byref(out)), b

    def frame_with(src, **fields):
        f = _lib.OrbFrame.from_buffer_copy(src)
        for k, v in fields.items():
            setattr(f, k, v)
        return f

    def kf2_with(**fields):
        arr = (_lib.OrbFrame * 2)(f2[0], f2[1])
        arr[1] = frame_with(f2[1], **fields)
        return arr

    n2 = [f.n for f in f2]
    INV = _lib.QSP_ERR_INVALID
    for kw in (dict(off2=[1, n2[0], n2[0] + n2[1]]), dict(off2=[-1, n2[0], n2[0] + n2[1]]), dict(off2=[0, n2[0], n2[0] - 1]),
               dict(off2=[0, n2[0], n2[0] + n2[1] + 1])):
        assert call(**kw)[0] == INV and untouched(), kw
    for name in ("kf1", "kf2", "off2", "K", "s12", "R12", "t12", "th", "pre1", "pre2"):
        assert call(drop_in=name)[0] == INV and untouched(), name
    for name in ("match12", "n_found", "best1", "dist2"):       # a partial tap is refused as well
        assert call(drop_out=name)[0] == INV and untouched(), name
    bad_oct = np.array(so.pool()[idx[1]]["kf2"]["octave"], np.int32)
    bad_oct[5] = so.N_LEVELS
    neg_oct = bad_oct.copy()
    neg_oct[5] = -1
    for fields in (dict(n=-1), dict(n=(1 << 26) + 1), dict(n_levels=17), dict(n_levels=0), dict(grid_cols=65), dict(grid_rows=0),
                   dict(octave=_lib.i32ptr(bad_oct)), dict(octave=_lib.i32ptr(neg_oct)), dict(kp=None), dict(mp_desc=None),
                   dict(scale_factors=None)):
        assert call(kf2=kf2_with(**fields))[0] == INV and untouched(), fields
    assert call(kf1=frame_with(f1, n_levels=17))[0] == INV and untouched()
    assert call(kf1=frame_with(f1, has_point=None))[0] == INV and untouched()
    assert call(n_cand=-1)[0] == INV and untouched()
    assert call(n_cand=0)[0] == _lib.QSP_OK and untouched()
    assert L.qsp_search_by_sim3_batch(0, C.byref(_lib.SearchSim3In()), None) == _lib.QSP_OK          # n_cand == 0 touches nothing
    assert L.qsp_search_by_sim3_batch(0, None, None) == INV
    # a NULL tap: the same match12 / n_found, the tap arrays untouched
    assert call(tap=False)[0] == _lib.QSP_OK
    n1 = f1.n
    for k, i in enumerate(idx):
        assert np.array_equal(o["match12"][k * n1:(k + 1) * n1], full[i]["match12"]) and o["n_found"][k] == full[i]["n_found"]
    assert all(np.array_equal(o[k], fresh[k]) for k in ("best1", "dist1", "best2", "dist2"))
    assert call()[0] == _lib.QSP_OK and not untouched()
    assert np.array_equal(o["best1"][:n1], full[idx[0]]["best1"]) and np.array_equal(o["dist2"][n2[0]:], full[idx[1]]["dist2"])


# ---- the mixed pool: every FrameP and CandP field differs between source and target and from one candidate to the next ---------
@pytest.fixture(scope="module")
def full_mixed():
    return run(so.pool_mixed())


def test_mixed_pool_equals_the_oracle_outside_its_band(full_mixed):
    """tests/test_oracle_search_sim3.py shows what a kernel that took the source's pyramid, candidate 0's K or th, rows for cols or
    an unclamped level would get wrong here (and that POOL lets four of the seven pass)"""
    width = so.band_mixed()
    margins.within("search_sim3/mixed/band_f32_vs_f64", so.measured_mixed(), width)
    worst, n_in_band, n_slots = 0.0, 0, 0
    for i, (r, g) in enumerate(zip(so.pool_mixed_results("f64"), full_mixed)):
        n_diff = 0
        for d in (1, 2):
            diff = (g["best%d" % d] != r["best%d" % d]) | (g["dist%d" % d] != r["dist%d" % d])
            n_diff += int(diff.sum())
            if diff.any():
                worst = max(worst, float(r["knife%d" % d][diff].max()))
            n_in_band += int((r["knife%d" % d] < width).sum())
            n_slots += len(diff)
        share = so.in_band_share(r, width)
        print("mixed candidate %d (%s): %d source slots differ from float64, %.4f of the slots inside the band"
              % (i, so.POOL_MIXED[i]["name"], n_diff, share))
        assert share <= so.IN_BAND_CAP, (i, share)
        # the agreement step, wherever both slots of the pair are outside the band
        sure = r["knife1"] >= width
        j = r["best1"]
        sure &= np.where(j >= 0, r["knife2"][np.maximum(j, 0)] >= width, True)
        assert np.array_equal(g["match12"][sure], r["match12"][sure]), i
        assert g["n_found"] == int((g["match12"] >= 0).sum())
        if sure.all():
            assert g["n_found"] == r["n_found"], (i, g["n_found"], r["n_found"])
    print("mixed pool: %d of %d source slots inside the band (undecided); largest knife-edge distance of a differing slot %.3e, "
          "BAND %.3e" % (n_in_band, n_slots, worst, width))
    margins.within("search_sim3/mixed/in_band_slots", n_in_band, so.IN_BAND_CAP * n_slots)
    assert margins.within("search_sim3/mixed/slot_edge", worst, width) and (worst < width or worst == 0.0)


def test_mixed_candidates_alone_reversed_and_between_the_old_ones(full_mixed):
    cands, old = so.pool_mixed(), so.pool()
    for i, c in enumerate(cands):                              # batches of 1: every candidate is candidate 0
        assert same_bits(run([c])[0], full_mixed[i]), i
    rev = run(cands[::-1])
    for i, (r, g) in enumerate(zip(rev[::-1], full_mixed)):
        assert same_bits(r, g), i
    woven = []                                                 # old, mixed, old, mixed ...: other frames and other K, th on both sides
    for i, c in enumerate(cands):
        woven += [old[i % len(old)], c]
    res = run(woven)
    for i in range(len(cands)):
        assert same_bits(res[2 * i + 1], full_mixed[i]), i
