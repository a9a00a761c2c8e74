"""GPU: qsp_search_for_triangulation_batch (SearchForTriangulation for all covisible neighbours in one call) against the literal
restatement of tests/search_triangulation_oracle.py.

Every output is an integer and every float operation a single IEEE operation, so there is no tolerance: match, match_raw, dist,
hist, ind and n_matches must be np.array_equal to the oracle on every fixture, with and without only_stereo and the orientation
check.  The count of differing slots is printed before it is asserted to be 0; a run with QSP_MARGINS_OUT lists it under
`search_triangulation/` (the committed copy: profiles/search_triangulation_margins.json).  The kernel has no size threshold; a
node of 4097 targets shows that a long list takes the same path."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import search_triangulation_oracle as to

pytestmark = pytest.mark.gpu


def run(shared, cands, F12, exy, tap=True, **p):
    from qsp_slam_amd.ba import search_for_triangulation_batch
    return search_for_triangulation_batch(shared, cands, F12, exy, tap=tap, **p)


def differing(got, want):
    return sum(int((got[k] != want[k]).sum()) for k in to.KEYS) + int(got["n_matches"] != want["n_matches"])


@pytest.mark.parametrize("only_stereo,ori", to.MODES)
def test_exact_equality_with_the_literal_oracle(only_stereo, ori):
    total = 0
    for name, (shared, cands, F12, exy) in to.scenes().items():
        got = run(shared, cands, F12, exy, only_stereo=bool(only_stereo), check_orientation=bool(ori))
        n = sum(differing(g, w) for g, w in zip(got, to.expected(name, only_stereo, ori)))
        print("%-20s only_stereo %d orientation %d: %d slots differ from the literal oracle" % (name, only_stereo, ori, n))
        margins.within("search_triangulation/differing_slots_%s" % name, n, 0)
        total += n
        for g in got:
            assert g["n_matches"] == int((g["match"] >= 0).sum())
    assert total == 0


def test_list_lengths_and_a_long_list_take_the_same_path():
    """lists of 0, 1, 63, 64, 65 and 129 targets are the `lengths` scene above; here a list of 4097, equal minima at its two ends"""
    nd = to.lengths_pair().named
    assert [len(nd["targets_%d" % n]) for n in to.LENGTHS] == [0, 1, 63, 64, 65, 129]
    for n_t in (4096, 4097):
        B = to.big_pair(n_t)
        src, tgt = B.frame(0), B.frame(1)
        want = to.literal(src, tgt, to.F_HAND, to.E_HAND)
        assert want["match_raw"][B.named["src"]] == B.named["last"] and want["ties"][B.named["src"]] == [0, n_t - 1]
        n = differing(run(src, [tgt], to.F_HAND[None], to.E_HAND[None])[0], want)
        print("%d targets in one node: %d slots differ" % (n_t, n))
        assert margins.within("search_triangulation/differing_slots_long_list", n, 0)


def test_alone_in_any_batch_at_any_position():
    shared, cands, F12, exy = to.scenes()["pool"]
    p = dict(check_orientation=True)
    full = run(shared, cands, F12, exy, **p)
    for i, c in enumerate(cands):                              # batches of 1
        assert to.same(run(shared, [c], F12[i:i + 1], exy[i:i + 1], **p)[0], full[i]), i
    for r, g in zip(run(shared, cands[::-1], F12[::-1], exy[::-1], **p)[::-1], full):       # every other position
        assert to.same(r, g)
    order = (None, 2, None, 5, 0, None)                        # next to empty candidates
    mixed = [to.EMPTY if i is None else cands[i] for i in order]
    sel = [0 if i is None else i for i in order]
    for r, i in zip(run(shared, mixed, F12[sel], exy[sel], **p), order):
        if i is None:
            assert r["n_matches"] == 0 and (r["match"] == -1).all() and (r["match_raw"] == -1).all()
        else:
            assert to.same(r, full[i]), i
    # NULL taps change nothing
    for r, g in zip(run(shared, cands, F12, exy, tap=False, **p), full):
        assert np.array_equal(r["match"], g["match"]) and r["n_matches"] == g["n_matches"] and "dist" not in r


def _raw(shared, cands):
    """the structs of a call, built by hand so that single fields can be broken"""
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _tri_frame
    keep = []
    f1 = _tri_frame(shared, keep, False)
    f2 = (_lib.TriFrame * len(cands))(*[_tri_frame(c, keep, True) for c in cands])
    n_out = len(cands) * f1.bow.n
    o = dict(match=np.full(n_out, -7, np.int32), n_matches=np.full(len(cands), -5, np.int32), match_raw=np.full(n_out, -3, np.int32),
             dist=np.full(n_out, -3, np.int32), hist=np.full(30 * len(cands), -3, np.int32), ind=np.full(3 * len(cands), -9, np.int32))
    return keep, f1, f2, o


def test_refusals_leave_the_outputs_untouched():
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import search_for_triangulation_batch
    shared, pool, F12, exy = to.scenes()["pool"]
    assert search_for_triangulation_batch(shared, [], np.zeros((0, 9)), np.zeros((0, 2))) == []
    L = _lib.lib()
    idx = [2, 5]
    cands = [pool[i] for i in idx]
    F, E = np.ascontiguousarray(F12[idx]).reshape(-1), np.ascontiguousarray(exy[idx]).reshape(-1)
    keep, f1, f2, o = _raw(shared, cands)
    fresh = {k: v.copy() for k, v in o.items()}
    untouched = lambda: all(np.array_equal(o[k], fresh[k]) for k in o)
    OUT = ("match", "n_matches", "match_raw", "dist", "hist", "ind")

    def call(n_cand=2, kf1=f1, kf2=f2, drop=(), th=50, ori=1):
        i = _lib.SearchTriIn(n_cand, None if "kf1" in drop else C.pointer(kf1), None if "kf2" in drop else kf2,
                             None if "F12" in drop else _lib.fptr(F), None if "exy" in drop else _lib.fptr(E), th, 0, ori)
        out = _lib.SearchTriOut(*[None if k in drop else _lib.i32ptr(o[k]) for k in OUT])
        return L.qsp_search_for_triangulation_batch(0, C.byref(i), C.byref(out))

    def frame_with(src, **fields):
        f = _lib.TriFrame.from_buffer_copy(src)
        for k, v in fields.items():
            setattr(f.bow if k in ("n", "n_nodes", "desc", "angle", "eligible", "node_id", "node_off", "feat") else f, k, v)
        return f

    def cand_with(**fields):
        arr = (_lib.TriFrame * 2)(f2[0], f2[1])
        arr[1] = frame_with(f2[1], **fields)
        return arr

    INV = _lib.QSP_ERR_INVALID
    c1 = cands[1]
    i32 = lambda a: np.array(a, np.int32)                                                # a copy: the fixtures are shared
    nn, nfeat = len(c1["node_id"]), len(c1["feat"])
    off_start = i32(c1["node_off"]); off_start[0] = 1
    off_dec = i32(c1["node_off"]); off_dec[2] = off_dec[1] - 1
    off_neg = i32(c1["node_off"]); off_neg[0] = -1
    ids_eq = i32(c1["node_id"]); ids_eq[3] = ids_eq[2]
    ids_desc = i32(c1["node_id"]); ids_desc[[2, 3]] = ids_desc[[3, 2]]
    feat_hi = i32(c1["feat"]); feat_hi[4] = len(c1["angle"])
    feat_neg = i32(c1["feat"]); feat_neg[4] = -1
    feat_twice = i32(c1["feat"]); feat_twice[nfeat - 1] = feat_twice[0]                  # the same index in two nodes
    assert nn > 4 and nfeat > 8
    for fields in (dict(n=-1), dict(n_nodes=-1), dict(desc=None), dict(angle=None), dict(node_id=None), dict(node_off=None), dict(feat=None),
                   dict(xy=None), dict(stereo=None), dict(sigma2=None), dict(scale=None),
                   dict(node_off=_lib.i32ptr(off_start)), dict(node_off=_lib.i32ptr(off_dec)), dict(node_off=_lib.i32ptr(off_neg)),
                   dict(node_id=_lib.i32ptr(ids_eq)), dict(node_id=_lib.i32ptr(ids_desc)), dict(feat=_lib.i32ptr(feat_hi)),
                   dict(feat=_lib.i32ptr(feat_neg)), dict(feat=_lib.i32ptr(feat_twice))):
        assert call(kf2=cand_with(**fields)) == INV and untouched(), fields
    for fields in (dict(node_off=None), dict(n=-2), dict(xy=None), dict(stereo=None)):
        assert call(kf1=frame_with(f1, **fields)) == INV and untouched(), fields
    for drop in ("kf1", "kf2", "F12", "exy", "match", "n_matches"):
        assert call(drop=(drop,)) == INV and untouched(), drop
    for th_bad in (-1, 257):
        assert call(th=th_bad) == INV and untouched()
    assert call(n_cand=-1) == INV and untouched()
    assert call(n_cand=0) == _lib.QSP_OK and untouched()                                 # n_cand == 0 touches nothing
    assert L.qsp_search_for_triangulation_batch(0, C.byref(_lib.SearchTriIn()), None) == _lib.QSP_OK
    assert L.qsp_search_for_triangulation_batch(0, None, None) == INV
    # more than 2^31 - 1 output slots in one call (n_cand * kf1's n; the work items, n_cand * kf1's list length, are never more):
    # refused before anything is staged
    many = 70000
    no_kp = [frame_with(f2[0], n=0, n_nodes=0)] * many
    zeros = np.zeros(9 * many, np.float32)
    out = _lib.SearchTriOut(_lib.i32ptr(o["match"]), _lib.i32ptr(o["n_matches"]), None, None, None, None)
    big = frame_with(f1, n=40000, n_nodes=0)
    i = _lib.SearchTriIn(many, C.pointer(big), (_lib.TriFrame * many)(*no_kp), _lib.fptr(zeros), _lib.fptr(zeros), 50, 0, 1)
    assert L.qsp_search_for_triangulation_batch(0, C.byref(i), C.byref(out)) == _lib.QSP_ERR_UNSUPPORTED and untouched()
    # the source's sigma2 and scale are not read: they are NULL here
    assert not f1.sigma2 and not f1.scale and call() == _lib.QSP_OK
    full = run(shared, cands, F12[idx], exy[idx], check_orientation=True)
    cat = lambda k: np.concatenate([r[k] for r in full])
    assert all(np.array_equal(o[k], cat(k)) for k in to.KEYS) and list(o["n_matches"]) == [r["n_matches"] for r in full]
    # each tap may be NULL on its own: the rest is written as in the full call
    for k in o:
        o[k][:] = fresh[k]
    assert call(drop=("dist", "ind")) == _lib.QSP_OK
    assert np.array_equal(o["dist"], fresh["dist"]) and np.array_equal(o["ind"], fresh["ind"])
    assert all(np.array_equal(o[k], cat(k)) for k in ("match", "match_raw", "hist"))
