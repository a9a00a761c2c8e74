"""GPU: qsp_fuse_batch (the match phase of both ORBmatcher::Fuse overloads for all target key frames in one call) against
tests/fuse_oracle.py.

best_idx, best_dist, reason and level must equal the float32 restatement on EVERY pair: 0 differing.  tests/test_oracle_fuse.py
holds the conditions on the fixtures under which that can be asked (no pair outside the deliberately exact ones sits on a
threshold).  A pair's outputs have the same bits alone, in any batch and at any list position.  A run with QSP_MARGINS_OUT lists
the counts under `fuse/` (the committed copy: profiles/fuse_margins.json)."""
import ctypes as C

import numpy as np
import pytest

from tests import fuse_oracle as fo
from tests import margins

pytestmark = pytest.mark.gpu

KEYS = ("best_idx", "best_dist", "reason", "level")


def run(targets, pool):
    from qsp_slam_amd.ba import fuse_batch
    return fuse_batch(targets, pool, tap=True)


@pytest.fixture(scope="module")
def full():
    return {which: run(*fo.scene(which)) for which in fo.SCENES}


def n_differing(g, r):
    return int(np.any([g[k] != r[k] for k in KEYS], axis=0).sum()) if len(r["reason"]) else 0


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize("which", fo.SCENES)
def test_every_pair_equals_the_restatement(full, which):
    """main: the pose overload, three targets with different n, n_levels, grids, K, th and pose, mono and stereo key points mixed,
    a permuted list, pool indices listed by several targets; sim3: the same without the reprojection test; stride: targets of 0, 1,
    63, 64, 65 and 4097 key points; exact: the cases that sit ON a threshold, under both overloads"""
    total = 0
    for k, (g, r) in enumerate(zip(full[which], fo.results(which))):
        n = n_differing(g, r)
        print("%s target %d (%d key points, %d pairs): %d pairs differ" % (which, k, len(fo.scene(which)[0][k]["octave"]), len(r["reason"]), n))
        total += n
    assert margins.within("fuse/%s/pairs_differing" % which, total, 0)


def test_ties_go_to_the_first_in_traversal_order(full):
    cases = fo.exact_scene()[2]
    for g in full["exact"]:
        for name in ("tie_cx", "tie_cy", "tie_cell"):
            c = cases[name]
            assert g["best_idx"][c["point"]] == c["best"] and g["best_dist"][c["point"]] == c["dist"], name
        assert cases["tie_cx"]["best"] != cases["tie_cx"]["lowest"] and cases["tie_cy"]["best"] != cases["tie_cy"]["lowest"]


def test_list_lengths_at_the_workgroup_edges(full):
    """lists of 0, 1, 3, 4 and 5 points (four waves per workgroup), alone and together in one call"""
    T, pool = fo.main_targets()[0], fo.main_pool()
    want = full["main"][0]
    cut = [dict(T, list=T["list"][:n]) for n in (0, 1, 3, 4, 5)]
    together = run(cut, pool)
    for t, g in zip(cut, together):
        n = len(t["list"])
        assert all(len(g[k]) == n and np.array_equal(g[k], want[k][:n]) for k in KEYS), n
        assert same_bits(run([t], pool)[0], g), n
    tail = dict(T, list=T["list"][-5:][::-1])                      # the last five, reversed: another position for each
    g = run([cut[2], tail], pool)[1]
    assert all(np.array_equal(g[k], want[k][-5:][::-1]) for k in KEYS)


@pytest.mark.parametrize("which", ("main", "exact", "stride"))
def test_alone_in_the_batch_and_reversed(full, which):
    targets, pool = fo.scene(which)
    for k, T in enumerate(targets):
        assert same_bits(run([T], pool)[0], full[which][k]), k
    rev = run(targets[::-1], pool)
    for k, (r, g) in enumerate(zip(rev[::-1], full[which])):
        assert same_bits(r, g), k
    if which == "main":                                            # both overloads in one call, woven
        woven = [t for pair in zip(targets, fo.sim3_targets()) for t in pair]
        res = run(woven, pool)
        for k in range(len(targets)):
            assert same_bits(res[2 * k], full["main"][k]) and same_bits(res[2 * k + 1], full["sim3"][k]), k


def test_refusals_leave_the_outputs_untouched(full):
    """every refusal of the contract (out-of-range indices are refused on the host, before any launch), and the empty calls"""
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import _fuse_in, fuse_batch
    assert fuse_batch([], fo.main_pool()) == []
    L = _lib.lib()
    targets, pool = [fo.main_targets()[0], fo.main_targets()[2]], fo.main_pool()
    i, keep, off = _fuse_in(targets, pool)
    arrays = keep[-1]
    n_pair = int(off[-1])
    o = {k: np.full(n_pair, -9, np.int32) for k in KEYS}
    untouched = lambda: all((v == -9).all() for v in o.values())
    INV, UNS, OK = _lib.QSP_ERR_INVALID, _lib.QSP_ERR_UNSUPPORTED, _lib.QSP_OK

    def call(inp=None, drop_out=None, tap=True):
        out = _lib.FuseOut(*[None if (k == drop_out or (not tap and k in ("reason", "level"))) else _lib.i32ptr(o[k]) for k in KEYS])
        return L.qsp_fuse_batch(0, C.byref(inp if inp is not None else i), C.byref(out))

    def with_(**fields):
        j = _lib.FuseIn.from_buffer_copy(i)
        for k, v in fields.items():
            setattr(j, k, v)
        return j

    def array_with(name, at, value):
        a = arrays[name].copy()
        a[at] = value
        keep.append(a)
        ptr = a.ctypes.data_as(C.POINTER(C.c_int64)) if a.dtype == np.int64 else _lib.i32ptr(a)
        return with_(**{name: ptr})

    def target_with(**fields):
        arr = (_lib.OrbFrame * 2)(i.target[0], i.target[1])
        f = _lib.OrbFrame.from_buffer_copy(i.target[1])
        for k, v in fields.items():
            setattr(f, k, v)
        arr[1] = f
        keep.append(arr)
        return with_(target=arr)

    for name in ("target", "K", "Ow", "th", "u_right_off", "u_right", "inv_level_sigma2", "check_reprojection", "Xw", "normal", "dist_min_inv",
                 "dist_max_inv", "dist_max", "desc", "list_off", "list_idx"):
        assert call(with_(**{name: None})) == INV and untouched(), name
    for name in ("best_idx", "best_dist", "reason", "level"):      # a partial tap is refused as well
        assert call(drop_out=name) == INV and untouched(), name
    assert call(with_(n_target=-1)) == INV and untouched()
    assert call(with_(n_point=-1)) == INV and untouched()
    n_point = len(pool["dist_max"])
    for inp in (array_with("list_off", 0, 1), array_with("list_off", 1, int(off[2]) + 1), array_with("list_idx", 3, n_point),
                array_with("list_idx", n_pair - 1, -1), array_with("u_right_off", 0, 1), array_with("u_right_off", 1, arrays["u_right_off"][1] + 1),
                with_(n_point=int(np.max(arrays["list_idx"]))), array_with("list_off", 2, int(off[1]) - 1)):
        assert call(inp) == INV and untouched()
    assert call(array_with("list_off", 2, 1 << 31)) == UNS and untouched()            # more than 2^31 - 1 pairs: refused before list_idx is read
    octs = np.array(targets[1]["octave"], np.int32)
    bad_oct, neg_oct = octs.copy(), octs.copy()
    bad_oct[5], neg_oct[5] = len(targets[1]["scale_factors"]), -1
    keep += [bad_oct, neg_oct]
    for fields in (dict(n=-1), dict(n=(1 << 26) + 1), dict(n_levels=17), dict(n_levels=0), dict(grid_cols=65), dict(grid_rows=0), dict(grid_cols=0),
                   dict(octave=_lib.i32ptr(bad_oct)), dict(octave=_lib.i32ptr(neg_oct)), dict(kp=None), dict(desc=None), dict(octave=None),
                   dict(scale_factors=None), dict(n=i.target[1].n - 1)):
        assert call(target_with(**fields)) == INV and untouched(), fields
    assert L.qsp_fuse_batch(0, None, None) == INV
    # the empty calls: no target; no listed pair (outputs may even be NULL)
    assert call(with_(n_target=0)) == OK and untouched()
    assert L.qsp_fuse_batch(0, C.byref(_lib.FuseIn()), None) == OK
    empty = np.zeros(3, np.int64)
    assert call(with_(list_off=empty.ctypes.data_as(C.POINTER(C.c_int64)))) == OK and untouched()
    assert L.qsp_fuse_batch(0, C.byref(with_(list_off=empty.ctypes.data_as(C.POINTER(C.c_int64)))), None) == OK
    # a NULL tap: the same best_idx / best_dist, the tap arrays untouched
    assert call(tap=False) == OK
    want = [full["main"][0], full["main"][2]]
    for k in ("best_idx", "best_dist"):
        assert np.array_equal(o[k], np.concatenate([w[k] for w in want])), k
    assert (o["reason"] == -9).all() and (o["level"] == -9).all()
    assert call() == OK
    for k in KEYS:
        assert np.array_equal(o[k], np.concatenate([w[k] for w in want])), k


def test_a_target_without_key_points_or_without_a_list_is_legal(full):
    targets, pool = fo.scene("stride")
    assert len(targets[0]["octave"]) == 0
    g = full["stride"][0]
    assert (g["best_idx"] == -1).all() and set(g["reason"]) <= {fo.Z_NEG, fo.OUTSIDE, fo.DISTANCE, fo.ANGLE, fo.EMPTY}
    none = dict(targets[3], list=np.zeros(0, np.int32))
    res = run([none, targets[3], none], pool)
    assert len(res[0]["best_idx"]) == 0 and len(res[2]["best_idx"]) == 0 and same_bits(res[1], full["stride"][3])
