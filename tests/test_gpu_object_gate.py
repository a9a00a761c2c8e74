"""GPU: the object map-point gate (qsp_object_gates, csrc/object_gate.hpp) against the numpy restatement in
tests/object_gate_oracle.py, on the fixtures of tests/object_gate_cases.py.

Flags (erased, outlier) and status equal the double flavour of the restatement exactly on every point whose knife-edge distance
is at least 1e-5; at most max(1, 0.5 %) of an object's points may be left out (tests/test_oracle_object_gate.py shows that the
fixtures themselves stay inside that cap).  whl, centre_w, R and T_wo_pca (R and the pose up to the joint sign of columns 0 and
2) lie within max(4 x the float32 flavour's own distance to the double flavour, 4 float32 ulps of the quantity's scale) of the
double flavour; the measured distances go to the margins table (tests/margins.py; committed: profiles/object_gate_margins.json)."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import object_gate_cases as GC
from tests import object_gate_oracle as GO

pytestmark = pytest.mark.gpu

FLIP = np.diag([-1.0, 1.0, -1.0])


@pytest.fixture(scope="module")
def gate():
    from qsp_slam_amd import _lib, gate_object_points, object_gate
    assert _lib.lib().qsp_device_count() > 0
    assert object_gate.LDS_POINTS == GC.LDS_POINTS
    return gate_object_points


@pytest.fixture(scope="module")
def cases():
    c = dict(GC.pca_cases())
    c.update(GC.model_cases())
    return c


@pytest.fixture(scope="module")
def gpu(gate, cases):
    """every fixture through ONE batched call"""
    names = list(cases)
    res = gate([{k: v for k, v in cases[n].items() if k != "expect"} for n in names])
    return dict(zip(names, res))


@pytest.fixture(scope="module")
def oracle(cases):
    return {n: (GO.gate(c, "f32"), GO.gate(c, "f64")) for n, c in cases.items()}


def _check_flags(name, g, ref):
    keep = ref["edge"] >= GC.BAND
    n = len(keep)
    assert np.count_nonzero(~keep) <= max(1, int(0.005 * n)), (name, "points inside the band", np.count_nonzero(~keep))
    assert g.status == ref["status"], (name, g.status, ref["status"])
    bad_e = np.nonzero((g.erased != ref["erased"]) & keep)[0]
    bad_o = np.nonzero((g.outlier != ref["outlier"]) & keep)[0]
    assert len(bad_e) == 0, (name, "erased differs at", bad_e[:8], ref["edge"][bad_e[:8]])
    assert len(bad_o) == 0, (name, "outlier differs at", bad_o[:8], ref["edge"][bad_o[:8]])


def _dist(a, b, flip):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b).max()
    if flip:
        a2 = a.copy()
        a2[:3, :3] = a[:3, :3] @ FLIP
        d = min(d, np.abs(a2 - b).max())
    return d


def _check_floats(name, g, f32, f64, pts, pca):
    cloud_scale = float(np.abs(pts).max())
    q = [("whl", np.array([g.w, g.h, g.l]), "whl", cloud_scale, False)]
    if pca:
        q += [("centre_w", g.centre_w, "centre_w", cloud_scale, False), ("R", g.R, "R", 1.0, True),
              ("T_wo_pca", g.T_wo, "T_wo", cloud_scale, True)]
    fails = []
    for label, val, key, scale, flip in q:
        assert np.all(np.isfinite(val)), (name, label)
        err = _dist(val, f64[key], flip)
        bar = max(4.0 * _dist(f32[key], f64[key], flip), 4.0 * float(np.spacing(np.float32(scale))))
        print("object_gate %s %s: gpu-f64 %.3e  f32-f64 %.3e  bar %.3e" % (name, label, err, _dist(f32[key], f64[key], flip), bar))
        if not margins.within("object_gate/%s/%s" % (name, label), err, bar):
            fails.append((label, err, bar))
    assert not fails, (name, fails)


PCA_NAMES = ["n%d" % n for n in GC.PCA_SIZES] + ["ties", "signed_zeros"]
MODEL_NAMES = ["mesh600", "verts11", "six_planes", "ymin_positive", "model_large"]


@pytest.mark.parametrize("name", PCA_NAMES)
def test_pca_against_the_restatement(name, gpu, oracle, cases):
    g, (f32, f64) = gpu[name], oracle[name]
    _check_flags(name, g, f64)
    assert g.status == GO.OK
    _check_floats(name, g, f32, f64, cases[name]["pts_world"], True)
    assert g.T_wo[3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_erase_pass_has_work(gpu):
    for n in GC.PCA_SIZES:
        if n > 10:
            assert np.count_nonzero(gpu["n%d" % n].erased) >= 2


@pytest.mark.parametrize("name", ["n2_all_erased", "n0_empty"])
def test_pca_bad(name, gpu, oracle):
    g = gpu[name]
    _check_flags(name, g, oracle[name][1])
    assert g.status == GO.BAD and (g.w, g.h, g.l) == (0.0, 0.0, 0.0) and not g.outlier.any()
    assert not g.R.any() and not g.centre_w.any() and not g.T_wo.any()
    if name == "n2_all_erased":
        assert g.erased.all()


def test_pca_three_coplanar_points(gate):
    """R is degenerate (the thin axis is free): status, erased, whl >= 0 and finite outputs only"""
    g = gate([GC.coplanar3()])[0]
    assert g.status == GO.OK and not g.erased.any()
    assert min(g.w, g.h, g.l) >= 0.0
    for a in (g.R, g.centre_w, g.T_wo, np.array([g.w, g.h, g.l])):
        assert np.all(np.isfinite(a))


def test_empty_object_between_two_full_ones(gate, gpu, cases):
    r = gate([cases["n65"], cases["n0_empty"], cases["n257"]])
    assert [x.status for x in r] == [GO.OK, GO.BAD, GO.OK]
    for a, b in ((r[0], gpu["n65"]), (r[2], gpu["n257"])):
        assert np.array_equal(a.outlier, b.outlier) and np.array_equal(a.erased, b.erased) and a.T_wo.tobytes() == b.T_wo.tobytes()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_against_the_restatement(name, gpu, oracle, cases):
    g, (f32, f64) = gpu[name], oracle[name]
    _check_flags(name, g, f64)
    assert g.status == GO.OK and not g.erased.any()
    assert g.R is None and g.centre_w is None and g.T_wo is None
    _check_floats(name, g, f32, f64, cases[name]["pts_world"], False)
    if name == "six_planes":
        assert np.array_equal(g.outlier, cases[name]["expect"])
    if name == "ymin_positive":       # the factor-on-extent reading would set other flags (tests/test_oracle_object_gate.py)
        assert 0 < np.count_nonzero(g.outlier) < len(g.outlier)


def test_model_ten_vertices_is_skipped(gpu):
    g = gpu["verts10_skipped"]
    assert g.status == GO.SKIPPED and not g.outlier.any() and not g.erased.any() and (g.w, g.h, g.l) == (0.0, 0.0, 0.0)


def _bytes(r):
    parts = [r.erased.tobytes(), r.outlier.tobytes(), np.array([r.w, r.h, r.l], np.float32).tobytes(), np.int32(r.status).tobytes()]
    parts += [b"" if a is None else a.tobytes() for a in (r.R, r.centre_w, r.T_wo)]
    return b"".join(parts)


def test_batch_invariance(gate):
    batch = GC.mixed_batch()
    assert len(batch) == 9
    whole = gate(batch)
    again = gate(batch)
    rev = gate(batch[::-1])[::-1]
    for i, o in enumerate(batch):
        alone = gate([o])[0]
        assert _bytes(whole[i]) == _bytes(alone), ("alone", i)
        assert _bytes(whole[i]) == _bytes(rev[i]), ("reversed", i)
        assert _bytes(whole[i]) == _bytes(again[i]), ("repeat", i)


# ---- the C-ABI's refusals -------------------------------------------------------------------------------------------------

SENT_U8, SENT_F, SENT_I = 0xA5, -77.0, -7


def _raw(n_obj, mode, pts_off, pts, T=None, vo=None, vv=None, null_in=False, null_out=False):
    from qsp_slam_amd import _lib
    n = max(int(n_obj), 1)
    npt = 16
    out = dict(erased=np.full(npt, SENT_U8, np.uint8), outlier=np.full(npt, SENT_U8, np.uint8), whl=np.full((n, 3), SENT_F, np.float32),
               R=np.full((n, 9), SENT_F, np.float32), centre_w=np.full((n, 3), SENT_F, np.float32),
               T_wo_pca=np.full((n, 16), SENT_F, np.float32), status=np.full(n, SENT_I, np.int32))
    keep = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in
            ((mode, np.int32), (pts_off, np.int32), (pts, np.float32), (T, np.float32), (vo, np.int32), (vv, np.float32))]
    ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_float)) for a in keep]
    gi = _lib.ObjectGateIn(n_obj=int(n_obj), mode=ptr[0], pts_off=ptr[1], pts_world=ptr[2], T_wo=ptr[3], vert_off=ptr[4], verts=ptr[5])
    go = _lib.ObjectGateOut(erased=_lib.u8ptr(out["erased"]), outlier=_lib.u8ptr(out["outlier"]), whl=_lib.fptr(out["whl"]),
                            R=_lib.fptr(out["R"]), centre_w=_lib.fptr(out["centre_w"]), T_wo_pca=_lib.fptr(out["T_wo_pca"]),
                            status=_lib.i32ptr(out["status"]))
    rc = _lib.lib().qsp_object_gates(0, None if null_in else C.byref(gi), None if null_out else C.byref(go))
    untouched = (np.all(out["erased"] == SENT_U8) and np.all(out["outlier"] == SENT_U8) and np.all(out["status"] == SENT_I) and
                 all(np.all(out[k] == SENT_F) for k in ("whl", "R", "centre_w", "T_wo_pca")))
    return rc, untouched


def test_refusals(gate):
    from qsp_slam_amd import _lib
    INV, UNS = _lib.QSP_ERR_INVALID, _lib.QSP_ERR_UNSUPPORTED
    pts = np.ones((16, 3), np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    vv = np.ones((12, 3), np.float32)
    ok2 = dict(mode=[0, 0], pts_off=[0, 8, 16], pts=pts)
    bad = {
        "null in": (INV, dict(ok2, null_in=True)),
        "null out": (INV, dict(ok2, null_out=True)),
        "null mode": (INV, dict(ok2, mode=None)),
        "null pts_off": (INV, dict(ok2, pts_off=None)),
        "null pts_world": (INV, dict(ok2, pts=None)),
        "negative count": (INV, dict(ok2, n_obj=-1)),
        "offsets start at 3": (INV, dict(ok2, pts_off=[3, 8, 16])),
        "offsets decrease": (INV, dict(ok2, pts_off=[0, 9, 8])),
        "mode 2": (INV, dict(ok2, mode=[0, 2])),
        "mode -1": (INV, dict(ok2, mode=[-1, 0])),
        "model without T_wo": (INV, dict(ok2, mode=[0, 1], vo=[0, 0, 12], vv=vv)),
        "model without vert_off": (INV, dict(ok2, mode=[0, 1], T=T, vv=vv)),
        "model without verts": (INV, dict(ok2, mode=[0, 1], T=T, vo=[0, 0, 12])),
        "vertex offsets decrease": (INV, dict(ok2, mode=[0, 1], T=T, vo=[0, 12, 11], vv=vv)),
        # 2^20 + 1 points by the offset table alone: refused before any point is read (the array holds 16)
        "2^20 + 1 points": (UNS, dict(ok2, pts_off=[0, 8, 8 + (1 << 20) + 1])),
    }
    for what, (code, kw) in bad.items():
        kw = dict(kw)
        n_obj = kw.pop("n_obj", 2)
        rc, untouched = _raw(n_obj, kw.pop("mode"), kw.pop("pts_off"), kw.pop("pts"), **kw)
        assert rc == code, (what, rc)
        assert untouched, what
    rc, untouched = _raw(0, None, None, None)
    assert rc == _lib.QSP_OK and untouched
    rc, untouched = _raw(2, **ok2)                   # the same arguments, valid: the sentinels go
    assert rc == _lib.QSP_OK and not untouched


# ---- the Python layer -----------------------------------------------------------------------------------------------------

class _Result:
    def __init__(self, vertices):
        self.vertices = vertices


def test_python_layer(gate, gpu, cases):
    from qsp_slam_amd import object_gate
    p, m = cases["n257"], cases["mesh600"]
    fort = np.asfortranarray(p["pts_world"].astype(np.float64))
    strided = np.zeros((len(m["pts_world"]), 6), np.float64)[:, ::2]
    strided[:] = m["pts_world"]
    assert m["vertices"].dtype == np.float64
    r = gate([dict(pts_world=fort),
              dict(pts_world=strided, vertices=_Result(m["vertices"]), T_wo=np.asfortranarray(m["T_wo"].astype(np.float64))),
              dict(pts_world=m["pts_world"], vertices=_Result(None), T_wo=m["T_wo"]),
              dict(pts_world=m["pts_world"], vertices=dict(vertices=m["vertices"], faces=None), T_wo=m["T_wo"])])
    assert _bytes(r[0]) == _bytes(gpu["n257"])
    assert _bytes(r[1]) == _bytes(gpu["mesh600"]) and _bytes(r[3]) == _bytes(gpu["mesh600"])
    assert r[2].status == GO.SKIPPED and not r[2].outlier.any()
    # the C-ABI call on flat arrays gives the same
    v32 = m["vertices"].astype(np.float32)
    flat = object_gate.object_gates([0, 1], [0, 257, 257 + len(m["pts_world"])], np.concatenate([p["pts_world"], m["pts_world"]]),
                                    np.stack([np.eye(4, dtype=np.float32), m["T_wo"]]), [0, 0, len(v32)], v32)
    assert flat["status"].tolist() == [GO.OK, GO.OK]
    assert np.array_equal(flat["outlier"][:257].astype(bool), r[0].outlier) and np.array_equal(flat["outlier"][257:].astype(bool), r[1].outlier)
    assert np.array_equal(flat["erased"][:257].astype(bool), r[0].erased)
    assert flat["whl"][0].tolist() == [r[0].w, r[0].h, r[0].l] and flat["whl"][1].tolist() == [r[1].w, r[1].h, r[1].l]
    assert flat["R"][0].tobytes() == r[0].R.tobytes() and flat["T_wo_pca"][0].tobytes() == r[0].T_wo.tobytes()
    assert not flat["R"][1].any() and not flat["T_wo_pca"][1].any()
    assert gate([]) == []
