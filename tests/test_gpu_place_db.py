"""GPU: the resident place-recognition database (qsp_place_db, include/qsp_hip.h; qsp_slam_amd.ba.PlaceDatabase) against the literal
restatement of tests/place_db_oracle.py.

The score is a serial double sum without products and everything after it single float32 operations and integer comparisons, so
there is no tolerance: every output and tap of query and accumulate must be np.array_equal to `Literal`, ids in order, float scores
compared as bits.  The count of differing entries is printed before it is asserted to be 0; a run with QSP_MARGINS_OUT lists it
under `place_db/` (the committed copy: profiles/place_db_margins.json).  The wave kernels have no size threshold; key frames and
queries of 63 / 64 / 65 / 4097 words stand at the wave edge and far beyond it.  The two single-workgroup kernels take entries 1024
at a time: 1023 / 1024 / 1025 / 2500 sharing key frames and entries stand on both sides of that."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import place_db_oracle as po

pytestmark = pytest.mark.gpu


class Device(object):
    """PlaceDatabase behind the interface of the oracles"""

    def __init__(self, **hints):
        from qsp_slam_amd.ba import PlaceDatabase
        self.db = PlaceDatabase(**hints)

    def put(self, kf_id, words, values, listed=True):
        self.db.put(kf_id, words, values, listed)

    def list(self, kf_id):
        self.db.list(kf_id)

    def erase(self, kf_id):
        self.db.erase(kf_id)

    def clear(self):
        self.db.clear()

    def detect(self, mode, words, values, neighbours, **kw):
        nb = lambda k: neighbours[k]
        if mode == po.LOOP:
            return self.db.detect_loop_candidates(words, values, nb, **kw)
        return self.db.detect_relocalization_candidates(words, values, nb)


def compare(name, ops, dev=None):
    dev = dev or Device()
    got, want = po.run_history(dev, ops), po.run_history(po.Literal(), ops)
    assert len(got) == len(want)
    n = sum(po.differing(g, w) for g, w in zip(got, want))
    print("%-50s %2d queries: %d entries differ from the literal oracle" % (name, len(want), n))
    ok = margins.within("place_db/differing_entries_%s" % name, n, 0)
    dev.db.close()
    return ok, got


@pytest.mark.parametrize("name", sorted(po.scenes()))
def test_exact_equality_with_the_literal_oracle(name):
    ok, got = compare(name, po.scenes()[name])
    assert ok


@pytest.mark.parametrize("n", po.LARGE_SIZES)
def test_beyond_one_pass_of_the_single_workgroup_kernels(n):
    """k_place_order ranks 1024 entries at a time against tiles of 1024 keys and k_place_acc strides by 1024: 1023 / 1024 / 1025 and
    2500 sharing key frames and entries of lScoreAndMatch stand on both sides of every tile edge, the partial last tile included"""
    ops = po.large_scene(n)
    ok, got = compare("large_%d" % n, ops)
    assert ok
    assert [g["n_sharing"] for g in got] == [n, n - 2, n, n - 1] and [len(g["acc_score"]) for g in got[2:]] == [n, n - 1]
    assert len(got[2]["cand_id"]) > 300 and list(got[2]["sharing_id"]) != sorted(got[2]["sharing_id"])


def test_the_stale_reloc_score():
    ops = po.stale_reloc_scene()
    ok, got = compare("stale_reloc_score_direct", ops)
    q1, q2 = got[0], got[1]
    assert ok and list(q2["match_id"]) == [1] and list(q2["sharing_id"]) == [1, 2]
    assert q2["acc_score"][0] == np.float32(q2["match_score"][0] + q1["match_score"][0])


def test_30_random_histories():
    bad = 0
    for seed in range(30):
        ok, _ = compare("random_histories", po.random_history(seed))
        bad += not ok
    assert bad == 0


def test_growing_the_arena_and_the_slots_from_a_small_capacity():
    from qsp_slam_amd.ba import PlaceDatabase
    dev = Device(words_hint=8, slots_hint=1)
    assert dev.db.size()["device_bytes"] < 1000
    ok, _ = compare("grown_from_8_words_1_slot", po.scenes()["wave_edges_63_64_65_4097"], dev)
    assert ok
    db = PlaceDatabase(words_hint=8, slots_hint=1)
    sizes = []
    for i in range(9):                                      # 9 x 5 words over 8: the arena doubles more than twice, the slots too
        db.put(i, np.arange(5) + i, np.full(5, 0.2))
        sizes.append(db.size()["device_bytes"])
    assert len(set(sizes)) >= 4 and db.size()["known"] == 9
    r = db.query(db.RELOC, np.arange(5), np.full(5, 0.2))
    assert list(r["sharing_id"]) == [0, 1, 2, 3, 4] and list(r["sharing_common"]) == [5, 4, 3, 2, 1]
    db.close()


def test_history_independence_and_clear():
    rng = np.random.default_rng(4)
    kfs = {i: po.bow(rng, int(rng.integers(4, 25)), 45) for i in range(12)}
    qv = po.bow(rng, 20, 45)
    nb = po.AnyNeighbours({i: [(i + 1) % 12, (i + 5) % 12, (i + 7) % 12] for i in range(12)})
    queries = [("query", po.LOOP, qv[0], qv[1], dict(excluded=[3], ref_ids=[0, 5]), nb), ("query", po.RELOC, qv[0], qv[1], {}, nb)]
    put = lambda i, listed=True: ("put", i, kfs[i][0], kfs[i][1], listed)
    direct = [put(i) for i in range(12)]
    # the same database and the same list order by another road: detours through erased key frames, late listing in order
    detour = [put(0), ("put", 77, kfs[3][0], kfs[3][1], True), put(1), ("erase", 77), ("put", 78, kfs[4][0], kfs[4][1], False), put(2), put(3),
              ("erase", 78), put(4, False), ("list", 4)] + [put(i) for i in range(5, 12)]
    a = po.run_history(Device(), direct + queries)
    b = po.run_history(Device(), detour + queries)
    n = sum(po.differing(x, y) for x, y in zip(a, b))
    print("two histories, one final database: %d entries differ" % n)
    assert margins.within("place_db/differing_entries_history_independence", n, 0)
    # another list order: what Literal gives for it
    other = [put(i) for i in range(11, -1, -1)]
    ok, c = compare("history_other_list_order", other + queries)
    assert ok and list(c[1]["sharing_id"]) != list(a[1]["sharing_id"]) and sorted(c[1]["sharing_id"]) == sorted(a[1]["sharing_id"])
    # after clear the handle equals a fresh one, persistent scores included
    dev = Device()
    po.run_history(dev, po.random_history(5) + po.stale_reloc_scene()[:3])
    dev.clear()
    assert dev.db.size()["known"] == 0 and dev.db.size()["listed"] == 0 and dev.db.size()["dead_slots"] == 0
    d = po.run_history(dev, direct + queries)
    n = sum(po.differing(x, y) for x, y in zip(d, a))
    print("after clear against a fresh handle: %d entries differ" % n)
    assert margins.within("place_db/differing_entries_after_clear", n, 0)


def test_size_reports_known_listed_and_holes():
    from qsp_slam_amd.ba import PlaceDatabase
    db = PlaceDatabase()
    w, v = np.arange(3), np.full(3, 1 / 3)
    db.put(1, w, v)
    db.put(2, w, v, listed=False)
    db.put(3, [], [])
    assert db.size()["known"] == 3 and db.size()["listed"] == 2 and db.size()["dead_slots"] == 0
    db.erase(2)
    db.erase(2)
    db.erase(12345)
    assert (db.size()["known"], db.size()["listed"], db.size()["dead_slots"]) == (2, 2, 1)
    db.put(2, w, v)                                         # an erased id is a new key frame
    assert (db.size()["known"], db.size()["listed"], db.size()["dead_slots"]) == (3, 3, 1)
    assert list(db.query(db.RELOC, w, v)["sharing_id"]) == [1, 2]
    db.close()


def test_refusals_leave_the_outputs_and_the_database_untouched():
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import PlaceDatabase
    L = _lib.lib()
    INV = _lib.QSP_ERR_INVALID
    rng = np.random.default_rng(9)
    db = PlaceDatabase()
    kfs = {i: po.bow(rng, 12, 30) for i in range(6)}
    for i in range(5):
        db.put(i, *kfs[i], listed=i != 4)
    qv = po.bow(rng, 14, 30)
    nb = {i: [(i + 1) % 5, (i + 2) % 5] for i in range(5)}
    base = db.detect_loop_candidates(qv[0], qv[1], nb, excluded=[1], ref_ids=[4, 0])
    assert len(base["match_id"]) >= 2
    h = db._h
    i32, f64, i64 = (lambda a: np.array(a, np.int32)), (lambda a: np.array(a, np.float64)), (lambda a: np.array(a, np.int64))

    def put(kf_id, n, w, v, listed=1):
        return L.qsp_place_db_put(h, kf_id, n, None if w is None else _lib.i32ptr(w), None if v is None else _lib.dptr(v), listed)

    w, v = i32(kfs[5][0]), f64(kfs[5][1])
    w_eq, w_desc, w_neg = w.copy(), w.copy(), w.copy()
    w_eq[3] = w_eq[2]
    w_desc[[2, 3]] = w_desc[[3, 2]]
    w_neg[0] = -1
    v_nan, v_inf = v.copy(), v.copy()
    v_nan[4], v_inf[5] = np.nan, -np.inf
    size0 = db.size()
    for args in ((5, -1, w, v), (5, 12, None, v), (5, 12, w, None), (5, 12, w_eq, v), (5, 12, w_desc, v), (5, 12, w_neg, v), (5, 12, w, v_nan),
                 (5, 12, w, v_inf), (0, 12, w, v), (4, 12, w, v)):
        assert put(*args) == INV, args[:2]
    assert L.qsp_place_db_put(None, 5, 0, None, None, 1) == INV
    assert L.qsp_place_db_list(h, 99) == INV and L.qsp_place_db_list(h, 0) == INV and L.qsp_place_db_list(None, 4) == INV
    assert L.qsp_place_db_erase(h, 99) == _lib.QSP_OK
    assert db.size() == size0

    cap = 8
    o = dict(match_id=np.full(cap, -7, np.int64), match_score=np.full(cap, -3, np.float32), sharing_id=np.full(cap, -7, np.int64),
             sharing_common=np.full(cap, -5, np.int32), sharing_first=np.full(cap, -9, np.int32), cand_id=np.full(cap, -7, np.int64),
             acc_score=np.full(cap, -3, np.float32), best_id=np.full(cap, -11, np.int64))
    fresh = {k: a.copy() for k, a in o.items()}
    qout = _lib.PlaceQueryOut(-1, -2, -3, -4, -5.0, _lib.i64ptr(o["match_id"]), _lib.fptr(o["match_score"]), _lib.i64ptr(o["sharing_id"]),
                              _lib.i32ptr(o["sharing_common"]), _lib.i32ptr(o["sharing_first"]))
    aout = _lib.PlaceAccOut(-6, _lib.i64ptr(o["cand_id"]), _lib.fptr(o["acc_score"]), _lib.i64ptr(o["best_id"]))

    def untouched():
        return (all(np.array_equal(o[k], fresh[k], equal_nan=True) for k in o) and aout.n_cand == -6
                and (qout.n_sharing, qout.max_common, qout.min_common, qout.n_match, qout.min_score_used) == (-1, -2, -3, -4, -5.0))

    qw, qx = i32(qv[0]), f64(qv[1])
    ex, rf = i64([1]), i64([4, 0])

    def query(mode=0, n=14, word=qw, value=qx, n_ex=1, excl=ex, min_score=0.0, n_ref=2, ref=rf, out=qout, handle=h):
        i = _lib.PlaceQueryIn(mode, n, None if word is None else _lib.i32ptr(word), None if value is None else _lib.dptr(value), n_ex,
                              None if excl is None else _lib.i64ptr(excl), min_score, n_ref, None if ref is None else _lib.i64ptr(ref))
        return L.qsp_place_db_query(handle, C.byref(i), None if out is None else C.byref(out))

    q_eq, q_neg, x_nan = qw.copy(), qw.copy(), qx.copy()
    q_eq[5] = q_eq[4]
    q_neg[0] = -4
    x_nan[0] = np.inf
    for kw in (dict(mode=2), dict(mode=-1), dict(n=-1), dict(word=None), dict(value=None), dict(word=q_eq), dict(word=q_neg), dict(value=x_nan),
               dict(n_ex=-1), dict(excl=None), dict(n_ref=-1), dict(ref=None), dict(ref=i64([4, 99])), dict(n_ref=0, min_score=float("nan")),
               dict(out=None), dict(handle=None)):
        assert query(**kw) == INV and untouched(), kw
    no_match = _lib.PlaceQueryOut(-1, -2, -3, -4, -5.0, None, _lib.fptr(o["match_score"]), None, None, None)
    assert query(out=no_match) == INV and untouched()
    # a live LOOP query, then refused accumulates
    assert query() == _lib.QSP_OK
    n = qout.n_match
    assert n == len(base["match_id"]) and np.array_equal(o["match_id"][:n], base["match_id"])
    assert np.array_equal(o["match_score"][:n].view(np.uint32), base["match_score"].view(np.uint32))
    ids = o["match_id"][:n].copy()
    snap = {k: a.copy() for k, a in o.items()}
    fresh.update(snap)
    qstate = (qout.n_sharing, qout.max_common, qout.min_common, qout.n_match, qout.min_score_used)
    untouched_acc = lambda: all(np.array_equal(o[k], snap[k]) for k in o) and aout.n_cand == -6
    off = i32(np.concatenate([[0], np.cumsum([len(nb[int(k)]) for k in ids])]))
    flat = i64([x for k in ids for x in nb[int(k)]])

    def acc(mode=0, n=n, ids=ids, off=off, flat=flat, out=aout, handle=h):
        return L.qsp_place_db_accumulate(handle, mode, n, None if ids is None else _lib.i64ptr(ids), None if off is None else _lib.i32ptr(off),
                                         None if flat is None else _lib.i64ptr(flat), None if out is None else C.byref(out))

    swapped = ids[::-1].copy()
    off_start, off_dec = off.copy(), off.copy()
    off_start[0] = 1
    off_dec[1] = off_dec[2] + 1 if n > 1 else -1
    for kw in (dict(mode=1), dict(mode=3), dict(n=-1), dict(n=n - 1), dict(ids=None), dict(ids=swapped), dict(off=None), dict(off=off_start),
               dict(off=off_dec), dict(flat=None), dict(out=None), dict(handle=None)):
        assert acc(**kw) == INV and untouched_acc(), kw
    no_cand = _lib.PlaceAccOut(-6, None, None, None)
    assert acc(out=no_cand) == INV and untouched_acc()
    assert acc() == _lib.QSP_OK and aout.n_cand == len(base["cand_id"])
    assert np.array_equal(o["cand_id"][:aout.n_cand], base["cand_id"]) and np.array_equal(o["best_id"][:n], base["best_id"])
    assert np.array_equal(o["acc_score"][:n].view(np.uint32), base["acc_score"].view(np.uint32))
    assert (qout.n_sharing, qout.max_common, qout.min_common, qout.n_match, qout.min_score_used) == qstate
    # a change of the database ends the query's life
    aout.n_cand = -6
    snap = {k: a.copy() for k, a in o.items()}
    db.put(5, *kfs[5])
    assert acc() == INV and untouched_acc()
    # NULL taps change nothing
    r = db.query(db.LOOP, qv[0], qv[1], excluded=[1], ref_ids=[4, 0], tap=False)
    assert "sharing_id" not in r and r["n_sharing"] >= n
    no_tap = _lib.PlaceAccOut(-6, _lib.i64ptr(o["cand_id"]), None, None)
    ids2 = i64(r["match_id"])
    off2 = i32(np.concatenate([[0], np.cumsum([len(nb.get(int(k), [])) for k in ids2])]))
    flat2 = i64([x for k in ids2 for x in nb.get(int(k), [])] + [0])
    assert acc(n=len(ids2), ids=ids2, off=off2, flat=flat2, out=no_tap) == _lib.QSP_OK and no_tap.n_cand >= 1
    assert np.array_equal(o["acc_score"], snap["acc_score"]) and np.array_equal(o["best_id"], snap["best_id"])
    db.close()
