"""GPU: qsp_triangulate_batch and qsp_create_new_map_points_batch (the numeric part of LocalMapping::CreateNewMapPoints for all
covisible neighbours in one call) against tests/triangulate_oracle.py.

Pairs on the two UnprojectStereo paths, and pairs that end before a 3-D point exists, must equal the float32 restatement bit for
bit: 0 differing, no tolerance.  (The issue excepts the stereo-cosine compare of pairs the oracle calls unstable; the fixtures hold
none, tests/test_oracle_triangulate.py asserts that, so nothing is excepted here.)  On the SVD path
the library computes the null vector in FP64 where the reference runs OpenCV's float32 SVD, so x3D is held to the pair's own noise
bar -- how far the reference's formulation moves under a one-ulp change of A, measured by the oracle alone -- and reason, path and
accept must be equal on every stable pair.  tests/test_oracle_triangulate.py holds the conditions on the fixtures.  A run with
QSP_MARGINS_OUT lists the counts and the largest distance / bar under `triangulate/` (the committed copy:
profiles/triangulate_margins.json)."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import search_triangulation_oracle as so
from tests import triangulate_oracle as to

pytestmark = pytest.mark.gpu

KEYS = to.SLOT_KEYS


def run(kf1, kf2s, match, tap=True):
    from qsp_slam_amd.ba import triangulate_batch
    return triangulate_batch(kf1, kf2s, match, tap=tap)


@pytest.fixture(scope="module")
def full():
    return {which: run(*to.scene(which)) for which in to.SCENES}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def differing(g, r, keys=KEYS):
    """per slot: any of the keys differs in its bits"""
    n = len(r["reason"])
    d = np.zeros(n, bool)
    for k in keys:
        d |= (bits(g[k]).reshape(n, -1) != bits(np.asarray(r[k]).astype(g[k].dtype)).reshape(n, -1)).any(axis=1)
    return d


def same_bits(a, b, keys=KEYS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


@pytest.mark.parametrize("which", to.SCENES)
def test_unproject_and_early_pairs_equal_the_restatement(full, which):
    total = 0
    for k, (g, r, nz) in enumerate(zip(full[which], to.results(which)[0], to.noise_of(which))):
        assert not nz["unstable"].any()
        exact = r["path"] != to.PATH_SVD
        n = int((differing(g, r) & exact).sum())
        print("%s neighbour %d: %d of %d pairs off the SVD path differ" % (which, k, n, exact.sum()))
        total += n
    assert margins.within("triangulate/%s/exact_pairs_differing" % which, total, 0)


@pytest.mark.parametrize("which", to.SCENES)
def test_svd_pairs_lie_within_their_noise_bar(full, which):
    worst, n_diff, n_svd = 0.0, 0, 0
    for k, (g, r, nz) in enumerate(zip(full[which], to.results(which)[0], to.noise_of(which))):
        svd = r["path"] == to.PATH_SVD
        n_svd += int(svd.sum())
        n_diff += int((differing(g, r, ("reason", "path", "accept")) & svd).sum())
        formed = svd & (r["reason"] != to.W_ZERO)
        if formed.any():
            d = np.abs(g["x3D"][formed].astype(np.float64) - r["x3D"][formed].astype(np.float64)).max(axis=1)
            ratio = d / nz["bar"][formed]
            print("%s neighbour %d: %d SVD pairs, largest |x3D - oracle| / bar %.3g (distance %.3g)" % (which, k, formed.sum(), ratio.max(), d.max()))
            worst = max(worst, float(ratio.max()))
    print("%s: %d stable SVD pairs, %d differ in reason / path / accept" % (which, n_svd, n_diff))
    if which == "exact":
        assert n_svd == 0
    ok_bar = margins.within("triangulate/%s/svd_distance_over_bar" % which, worst, 1.0)
    ok_diff = margins.within("triangulate/%s/svd_stable_pairs_differing" % which, n_diff, 0)
    assert ok_bar and ok_diff


def test_w_zero_ends_the_pair_before_a_point_exists(full):
    """the null vector's w is exactly 0 (a zero first column in both Rcw): reason 3 on the SVD path, no point, every tap but the
    rays' cosine untouched, bit for bit the oracle's"""
    g, r = full["w_zero"][0], to.results("w_zero")[0][0]
    assert list(g["reason"]) == [to.W_ZERO, to.W_ZERO] and list(g["path"]) == [to.PATH_SVD, to.PATH_SVD]
    assert not g["accept"].any() and not g["first"].any() and g["n_new"] == 0 and not g["x3D"].any()
    assert not differing(g, r).any()


def test_the_exact_cases(full):
    _, _, _, cases = to.exact_scene()
    for name, c in cases.items():
        k, i, want = c[:3]
        assert full["exact"][k]["reason"][i] == want, name
        if len(c) == 4:
            assert full["exact"][k]["err2"][i, 0] == c[3], name


@pytest.mark.parametrize("which", to.SCENES)
def test_first_is_the_first_accepted(full, which):
    acc = np.stack([g["accept"] for g in full[which]])
    fst = np.stack([g["first"] for g in full[which]])
    assert np.array_equal(fst, to.first_rule(acc))
    assert [g["n_new"] for g in full[which]] == [int(f.sum()) for f in fst]
    if which == "order":
        assert np.array_equal(fst, np.stack([r["first"] for r in to.results("order")[0]]))
        assert fst.sum() == 4 and (acc & ~fst).sum() == 1


@pytest.mark.parametrize("n_cand,n1", to.EDGE_COUNTS)
def test_slot_counts_at_the_workgroup_edges(n_cand, n1):
    for at_last in (False, True):
        kf1, nbs, m = to.edge_scene(n_cand, n1, at_last)
        got = run(kf1, nbs, m)
        want = to.triangulate(kf1, nbs, m)[0]
        assert len(got) == n_cand
        for g, r in zip(got, want):
            assert len(g["accept"]) == n1
            assert not differing(g, r, ("reason", "path", "accept", "first", "cos_rays")).any()
            assert g["n_new"] == r["n_new"]
        if n_cand * n1:
            assert sum(g["n_new"] for g in got) == 1 and got[-1 if at_last else 0]["first"][-1 if at_last else 0]


def test_a_key_frame_without_key_points():
    """neighbours, but no slot: nothing is launched, n_new is 0 for every neighbour; in the chained call the search still reports"""
    from qsp_slam_amd.ba import create_new_map_points_batch
    kf1, nbs, m = to.edge_scene(2, 0, False)
    got = run(kf1, nbs, m)
    assert [g["n_new"] for g in got] == [0, 0] and all(len(g["accept"]) == 0 and g["x3D"].shape == (0, 3) for g in got)
    shared, cands, F12, exy = so.scenes()["source_empty"]
    got = create_new_map_points_batch(to.with_geometry(shared, 0), [to.with_geometry(c, 1 + i) for i, c in enumerate(cands)], F12, exy, tap=True)
    assert [g["n_new"] for g in got] == [0, 0] and [g["n_matches"] for g in got] == [0, 0] and all(len(g["first"]) == 0 for g in got)


def test_alone_in_the_batch_and_reversed(full):
    kf1, kf2s, match = to.scene("main")
    for k, f in enumerate(kf2s):
        assert same_bits(run(kf1, [f], match[k:k + 1])[0], full["main"][k]), k
    rev = run(kf1, kf2s[::-1], match[::-1])
    for k, (r, g) in enumerate(zip(rev[::-1], full["main"])):
        assert same_bits(r, g), k
    none = np.full((1, match.shape[1]), -1, np.int32)
    woven = run(kf1, [kf2s[2], kf2s[0], kf2s[1]], np.concatenate([none, match[0:1], match[1:2]]))
    assert not woven[0]["accept"].any() and (woven[0]["reason"] == to.NO_MATCH).all() and woven[0]["n_new"] == 0
    assert same_bits(woven[1], full["main"][0]) and same_bits(woven[2], full["main"][1])
    assert np.array_equal(np.stack([w["first"] for w in woven[1:]]), np.stack([g["first"] for g in run(kf1, kf2s[:2], match[:2])]))


@pytest.mark.parametrize("only_stereo,ori", so.MODES)
def test_the_chained_call_equals_the_two_calls(only_stereo, ori):
    from qsp_slam_amd.ba import create_new_map_points_batch, search_for_triangulation_batch
    shared, cands, F12, exy = so.scenes()["pool"]
    kf1 = to.with_geometry(shared, 0)
    kf2s = [to.with_geometry(c, 1 + i) for i, c in enumerate(cands)]
    p = dict(only_stereo=bool(only_stereo), check_orientation=bool(ori), tap=True)
    found = search_for_triangulation_batch(kf1, kf2s, F12, exy, **p)
    match = np.stack([f["match"] for f in found])
    want = run(kf1, kf2s, match)
    got = create_new_map_points_batch(kf1, kf2s, F12, exy, **p)
    n_acc = 0
    for k, (g, f, w) in enumerate(zip(got, found, want)):
        assert so.same(g, f), k
        assert same_bits(g, w, KEYS + ("first",)) and g["n_new"] == w["n_new"], k
        n_acc += int(g["accept"].sum())
    print("only_stereo %d orientation %d: %d matches, %d accepted" % (only_stereo, ori, (match >= 0).sum(), n_acc))
    assert (match >= 0).sum() > 0
    quiet = create_new_map_points_batch(kf1, kf2s, F12, exy, only_stereo=bool(only_stereo), check_orientation=bool(ori))
    for q, g in zip(quiet, got):
        assert np.array_equal(q["match"], g["match"]) and same_bits(q, g, ("accept", "first", "x3D")) and "reason" not in q


def test_refusals_leave_the_outputs_untouched(full):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _TRI_TAPS, _tri_frame, _triangulate_geom, create_new_map_points_batch, triangulate_batch
    L = _lib.lib()
    INV, UNS, OK = _lib.QSP_ERR_INVALID, _lib.QSP_ERR_UNSUPPORTED, _lib.QSP_OK
    kf1, kf2s, match = to.scene("main")
    assert triangulate_batch(kf1, [], np.zeros((0, 300), np.int32)) == []
    keep = []
    g = _triangulate_geom(kf1, kf2s, keep)
    nc, n1 = len(kf2s), len(kf1["u_right"])
    m = np.ascontiguousarray(match.reshape(-1), np.int32)
    a = dict(accept=np.full(nc * n1, 9, np.uint8), first=np.full(nc * n1, 9, np.uint8), x3D=np.full(3 * nc * n1, -9, np.float32),
             n_new=np.full(nc, -9, np.int32))
    a.update({k: np.full(w * nc * n1, -9, dt) for k, dt, w in _TRI_TAPS})
    clean = {k: v.copy() for k, v in a.items()}
    untouched = lambda: all(np.array_equal(a[k], clean[k]) for k in a)
    P = dict(accept=_lib.u8ptr, first=_lib.u8ptr, x3D=_lib.fptr, n_new=_lib.i32ptr, reason=_lib.i32ptr, path=_lib.i32ptr, cos_rays=_lib.fptr,
             z=_lib.fptr, err2=_lib.fptr, ratio_dist=_lib.fptr)

    def out(drop=()):
        return _lib.TriangulateOut(**{k: (None if k in drop else P[k](a[k])) for k in P})

    def call(geom=None, mm=m, o=None, null_out=False):
        return L.qsp_triangulate_batch(0, C.byref(geom if geom is not None else g), None if mm is None else _lib.i32ptr(mm),
                                       None if null_out else C.byref(o if o is not None else out()))

    def geom_with(**fields):
        j = _lib.TriangulateGeom.from_buffer_copy(g)
        for k, v in fields.items():
            setattr(j, k, v)
        return j

    def frame_with(which, **fields):
        arr = (_lib.TriangulateFrame * nc)(*[g.kf2[k] for k in range(nc)])
        f = _lib.TriangulateFrame.from_buffer_copy(g.kf1[0] if which < 0 else g.kf2[which])
        for k, v in fields.items():
            setattr(f, k, v)
        keep.extend([arr, f])
        if which < 0:
            return geom_with(kf1=C.pointer(f))
        arr[which] = f
        return geom_with(kf2=arr)

    assert L.qsp_triangulate_batch(0, None, _lib.i32ptr(m), C.byref(out())) == INV and untouched()
    assert call(null_out=True) == INV
    assert call(mm=None) == INV and untouched()
    for name in ("accept", "first", "x3D", "n_new"):
        assert call(o=out(drop=(name,))) == INV and untouched(), name
    assert call(geom_with(n_cand=-1)) == INV and untouched()
    assert call(geom_with(kf1=None)) == INV and untouched()
    assert call(geom_with(kf2=None)) == INV and untouched()
    for which in (-1, 1):
        assert call(frame_with(which, n=-1)) == INV and untouched()
        for name in ("xy_un", "xy", "u_right", "depth", "sigma2", "scale"):
            assert call(frame_with(which, **{name: None})) == INV and untouched(), name
    for at, v in ((0, -2), (n1 + 5, len(kf2s[1]["u_right"])), (nc * n1 - 1, 1 << 30)):
        bad = m.copy()
        bad[at] = v
        assert call(mm=bad) == INV and untouched(), at
    assert call(frame_with(1, n=int(match[1].max()))) == INV and untouched()              # an index the neighbour no longer holds
    assert call(frame_with(-1, n=1 << 30)) == UNS and untouched()                          # 3 * 2^30 slots: refused before any array is read
    # the empty calls
    assert call(geom_with(n_cand=0)) == OK and untouched()
    assert L.qsp_triangulate_batch(0, C.byref(_lib.TriangulateGeom()), None, None) == OK
    # NULL taps: the same accept / first / x3D / n_new, the tap arrays untouched
    assert call(o=out(drop=[k for k, _, _ in _TRI_TAPS])) == OK
    want = full["main"]
    for k in ("accept", "first"):
        assert np.array_equal(a[k].astype(bool), np.concatenate([w[k] for w in want])), k
    assert np.array_equal(bits(a["x3D"]), bits(np.concatenate([w["x3D"] for w in want]).reshape(-1)))
    assert list(a["n_new"]) == [w["n_new"] for w in want]
    assert all(np.array_equal(a[k], clean[k]) for k, _, _ in _TRI_TAPS)
    assert call(o=out(drop=("path", "z"))) == OK                                           # any subset of the taps
    assert np.array_equal(a["reason"], np.concatenate([w["reason"] for w in want])) and np.array_equal(a["path"], clean["path"])
    # the chained call: what either half refuses, and frames that differ between the two inputs
    shared, cands, F12, exy = so.scenes()["pool"]
    s1, s2 = to.with_geometry(shared, 0), [to.with_geometry(c, 1 + i) for i, c in enumerate(cands[:2])]
    f1 = _tri_frame(s1, keep, False)
    f2 = (_lib.TriFrame * 2)(*[_tri_frame(c, keep, True) for c in s2])
    F, e = np.ascontiguousarray(F12[:2], np.float32), np.ascontiguousarray(exy[:2], np.float32)
    si = _lib.SearchTriIn(2, C.pointer(f1), f2, _lib.fptr(F), _lib.fptr(e), 50, 0, 0)
    gg = _triangulate_geom(s1, s2, keep)
    n = 2 * len(s1["u_right"])
    sm, sc = np.full(n, -9, np.int32), np.full(2, -9, np.int32)
    so_ = _lib.SearchTriOut(_lib.i32ptr(sm), _lib.i32ptr(sc))
    chained = lambda i=si, q=gg, o1=so_, o2=None: L.qsp_create_new_map_points_batch(0, C.byref(i) if i is not None else None,
                                                                                     C.byref(q) if q is not None else None, C.byref(o1),
                                                                                     C.byref(o2 if o2 is not None else out()))
    still = lambda: untouched() and (sm == -9).all() and (sc == -9).all()
    a.update({k: v.copy() for k, v in clean.items()})
    assert chained(i=None) == INV and chained(q=None) == INV and still()
    g3 = _lib.TriangulateGeom.from_buffer_copy(gg)
    g3.n_cand = 1
    assert chained(q=g3) == INV and still()
    assert chained(q=g) == INV and still()                                                  # three neighbours against two
    short = dict(s2[1])
    for k, w in (("xy", 2), ("xy_raw", 2), ("u_right", 1), ("depth", 1), ("sigma2", 1), ("scale", 1)):
        short[k] = np.asarray(short[k])[:-1]
    assert chained(q=_triangulate_geom(s1, [s2[0], short], keep)) == INV and still()        # a frame one key point shorter in the geometry
    bad_th = _lib.SearchTriIn.from_buffer_copy(si)
    bad_th.th = 257
    assert chained(i=bad_th) == INV and still()
    assert chained(o2=out(drop=("first",))) == INV and still()
    assert chained(o1=_lib.SearchTriOut(None, _lib.i32ptr(sc))) == INV and still()
    raw = L.qsp_create_new_map_points_batch
    assert raw(0, C.byref(si), C.byref(gg), None, C.byref(out())) == INV and still()                 # a null output of either half
    assert raw(0, C.byref(si), C.byref(gg), C.byref(so_), None) == INV and still()
    neg_i, neg_g = _lib.SearchTriIn.from_buffer_copy(si), _lib.TriangulateGeom.from_buffer_copy(gg)
    neg_i.n_cand = neg_g.n_cand = -1
    assert chained(i=neg_i) == INV and chained(q=neg_g) == INV and chained(i=neg_i, q=neg_g) == INV and still()
    huge = _lib.TriangulateFrame.from_buffer_copy(gg.kf1[0])
    huge.n = 1 << 30                                                                                  # 2 * 2^30 slots: decided on the counts alone
    keep.append(huge)
    big = _lib.TriangulateGeom.from_buffer_copy(gg)
    big.kf1 = C.pointer(huge)
    assert chained(q=big) == UNS and still()
    zero_i, zero_g = _lib.SearchTriIn.from_buffer_copy(si), _lib.TriangulateGeom.from_buffer_copy(gg)
    zero_i.n_cand = zero_g.n_cand = 0
    assert chained(i=zero_i, q=zero_g) == OK and still()                                              # the empty call touches nothing
    assert create_new_map_points_batch(s1, [], F12[:0], exy[:0]) == []
