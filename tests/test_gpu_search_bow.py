"""GPU: qsp_search_by_bow_batch (SearchByBoW for all loop or relocalisation candidates in one call) against the literal
restatement of tests/search_bow_oracle.py.

Every output is an integer and every float operation a single IEEE float32 operation, so there is no tolerance: match, match_raw,
dist, hist, ind and n_matches must be np.array_equal to the oracle on every fixture, in both modes, with and without the
orientation check.  The count of differing slots is printed before it is asserted to be 0; a run with QSP_MARGINS_OUT lists it
under `search_bow/` (the committed copy: profiles/search_bow_margins.json).  The kernel has no size threshold (the taken marks of
any node size live in one scratch array); a node of 4097 targets shows that a long list takes the same path."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import search_bow_oracle as bo

pytestmark = pytest.mark.gpu


def run(shared, cands, sis, check_orientation=True, tap=True, **p):
    from qsp_slam_amd.ba import search_by_bow_batch
    return search_by_bow_batch(shared, cands, shared_is_source=sis, check_orientation=check_orientation, tap=tap, **p)


def differing(got, want):
    return sum(int((got[k] != want[k]).sum()) for k in bo.KEYS) + int(got["n_matches"] != want["n_matches"])


@pytest.mark.parametrize("ori", [1, 0])
def test_exact_equality_with_the_literal_oracle(ori):
    total = 0
    for name, (shared, cands, sis) in bo.scenes().items():
        for pi, p in enumerate(bo.params_of(name)):
            got = run(shared, cands, sis, bool(ori), **p)
            n = sum(differing(g, w) for g, w in zip(got, bo.expected(name, pi, ori)))
            print("%-26s params %d orientation %d: %d slots differ from the literal oracle" % (name, pi, ori, n))
            margins.within("search_bow/differing_slots_%s" % name.split("_")[0], n, 0)
            total += n
            for g in got:
                assert g["n_matches"] == int((g["match"] >= 0).sum())
    assert total == 0


def test_a_long_target_list_takes_the_same_path():
    for n_t in (4096, 4097):
        B = bo.big_pair(n_t)
        for sis in (True, False):
            src, tgt = B.frame(0), B.frame(1, all_eligible=not sis)
            shared, cands = (src, [tgt]) if sis else (tgt, [src])
            want = bo.literal(shared, cands[0], shared_is_source=sis)
            nd = B.named
            assert want["match_raw"][nd["first"]] == nd["last"] and want["match_raw"][nd["second"]] == nd["middle"]      # the steal
            assert want["info"][nd["second"]]["stolen"] and want["match_raw"][nd["third"]] == -1
            n = differing(run(shared, cands, sis)[0], want)
            print("%d targets in one node, shared_is_source %d: %d slots differ" % (n_t, sis, n))
            assert margins.within("search_bow/differing_slots_long_list", n, 0)


@pytest.mark.parametrize("name", ["kf_pool", "frame_pool"])
def test_alone_in_any_batch_at_any_position(name):
    shared, cands, sis = bo.scenes()[name]
    p = bo.params_of(name)[0]
    same = lambda a, b: bo.same(a, b)
    full = run(shared, cands, sis, **p)
    for i, c in enumerate(cands):                              # batches of 1
        assert same(run(shared, [c], sis, **p)[0], full[i]), i
    for r, g in zip(run(shared, cands[::-1], sis, **p)[::-1], full):       # every other position
        assert same(r, g)
    empty = bo.make_frame(np.zeros((0, 32), np.uint8), [], [])
    mixed = [empty, cands[2], empty, cands[5], cands[0], empty]            # next to empty candidates
    for r, i in zip(run(shared, mixed, sis, **p), (None, 2, None, 5, 0, None)):
        if i is None:
            assert r["n_matches"] == 0 and len(r["match"]) == 0 if not sis else (r["match"] == -1).all()
        else:
            assert same(r, full[i]), i
    # NULL taps change nothing
    for r, g in zip(run(shared, cands, sis, tap=False, **p), full):
        assert np.array_equal(r["match"], g["match"]) and r["n_matches"] == g["n_matches"] and "dist" not in r


def _raw(shared, cands, sis):
    """the structs of a call, built by hand so that single fields can be broken"""
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _bow_frame
    keep = []
    f0 = _bow_frame(shared, keep)
    fc = (_lib.BowFrame * len(cands))(*[_bow_frame(c, keep) for c in cands])
    n_out = len(cands) * f0.n if sis else sum(f.n for f in fc)
    o = dict(match=np.full(n_out, -7, np.int32), n_matches=np.full(len(cands), -5, np.int32), match_raw=np.full(n_out, -3, np.int32),
             dist=np.full(n_out, -3, np.int32), hist=np.full(30 * len(cands), -3, np.int32), ind=np.full(3 * len(cands), -9, np.int32))
    return keep, f0, fc, o


@pytest.mark.parametrize("name", ["kf_pool", "frame_pool"])
def test_refusals_leave_the_outputs_untouched(name):
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import search_by_bow_batch
    shared, pool, sis = bo.scenes()[name]
    assert search_by_bow_batch(shared, [], shared_is_source=sis) == []
    L = _lib.lib()
    idx = (2, 6)
    cands = [pool[i] for i in idx]
    keep, f0, fc, o = _raw(shared, cands, sis)
    fresh = {k: v.copy() for k, v in o.items()}
    untouched = lambda: all(np.array_equal(o[k], fresh[k]) for k in o)
    p = bo.params_of(name)[0]

    def call(n_cand=2, shared_f=f0, cand_f=fc, drop=(), th=p["th"], nn=p["nn_ratio"]):
        i = _lib.SearchBowIn(n_cand, 1 if sis else 0, None if "shared" in drop else C.pointer(shared_f), None if "cand" in drop else cand_f,
                             th, 1 if p["th_inclusive"] else 0, nn, 1)
        out = _lib.SearchBowOut(*[None if k in drop else _lib.i32ptr(o[k]) for k in ("match", "n_matches", "match_raw", "dist", "hist", "ind")])
        return L.qsp_search_by_bow_batch(0, C.byref(i), C.byref(out))

    def frame_with(src, **fields):
        f = _lib.BowFrame.from_buffer_copy(src)
        for k, v in fields.items():
            setattr(f, k, v)
        return f

    def cand_with(**fields):
        arr = (_lib.BowFrame * 2)(fc[0], fc[1])
        arr[1] = frame_with(fc[1], **fields)
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
                   dict(node_off=_lib.i32ptr(off_start)), dict(node_off=_lib.i32ptr(off_dec)), dict(node_off=_lib.i32ptr(off_neg)),
                   dict(node_id=_lib.i32ptr(ids_eq)), dict(node_id=_lib.i32ptr(ids_desc)), dict(feat=_lib.i32ptr(feat_hi)),
                   dict(feat=_lib.i32ptr(feat_neg)), dict(feat=_lib.i32ptr(feat_twice))):
        assert call(cand_f=cand_with(**fields)) == INV and untouched(), fields
    assert call(shared_f=frame_with(f0, node_off=None)) == INV and untouched()
    assert call(shared_f=frame_with(f0, n=-2)) == INV and untouched()
    for drop in ("shared", "cand", "match", "n_matches"):
        assert call(drop=(drop,)) == INV and untouched(), drop
    for nn_bad in (float("nan"), float("inf"), -float("inf")):
        assert call(nn=nn_bad) == INV and untouched()
    for th_bad in (-1, 257):
        assert call(th=th_bad) == INV and untouched()
    assert call(n_cand=-1) == INV and untouched()
    assert call(n_cand=0) == _lib.QSP_OK and untouched()                                 # n_cand == 0 touches nothing
    assert L.qsp_search_by_bow_batch(0, C.byref(_lib.SearchBowIn()), None) == _lib.QSP_OK
    assert L.qsp_search_by_bow_batch(0, None, None) == INV
    # more than 2^31 - 1 output slots in one call (n_cand * shared->n), refused before anything is read
    many = 70000
    big = frame_with(f0, n=40000, n_nodes=0)
    i = _lib.SearchBowIn(many, 1 if sis else 0, C.pointer(big), (_lib.BowFrame * many)(*([frame_with(fc[0], n=0, n_nodes=0)] * many)),
                         50, 0, 0.75, 1)
    out = _lib.SearchBowOut(_lib.i32ptr(o["match"]), _lib.i32ptr(o["n_matches"]), None, None, None, None)
    assert L.qsp_search_by_bow_batch(0, C.byref(i), C.byref(out)) == _lib.QSP_ERR_UNSUPPORTED and untouched()
    # each tap may be NULL on its own: the rest is written as in the full call
    full = run(shared, cands, sis, **p)
    assert call(drop=("dist", "ind")) == _lib.QSP_OK
    assert np.array_equal(o["dist"], fresh["dist"]) and np.array_equal(o["ind"], fresh["ind"])
    assert np.array_equal(o["match"], np.concatenate([r["match"] for r in full]))
    assert np.array_equal(o["match_raw"], np.concatenate([r["match_raw"] for r in full]))
    assert np.array_equal(o["hist"], np.concatenate([r["hist"] for r in full])) and list(o["n_matches"]) == [r["n_matches"] for r in full]
    assert call() == _lib.QSP_OK and np.array_equal(o["ind"], np.concatenate([r["ind"] for r in full]))
    assert np.array_equal(o["dist"], np.concatenate([r["dist"] for r in full]))
