"""GPU: qsp_sim3_ransac_batch (Sim3Solver for all loop candidates in one call) against tests/sim3_ransac_oracle.py.

The inlier flags of EVERY hypothesis (read by running each as a candidate of its own with min_inliers = -1, which batch
independence makes the same bits) must equal the float64 flavour's on every (hypothesis, match) pair whose knife-edge distance is
at least BAND = 4 x the band measured on the CPU between the oracle's two flavours; the per-hypothesis counts of the tap must lie
between the sure inliers and sure plus in-band; the first success must be the oracle's; R, t, s must lie within max(4 x the
float32 flavour's own distance to float64 on that winning hypothesis, 4 float32 ulps of the quantity's scale).
tests/test_oracle_sim3_ransac.py holds the conditions on the fixtures under which the band decides nothing.  A candidate's outputs have the same bits alone, in any batch
and at any position.  Every figure is printed before it is asserted; a run with QSP_MARGINS_OUT lists them under `sim3_ransac/`
(the committed copy: profiles/sim3_ransac_margins.json)."""
import numpy as np
import pytest

from tests import margins
from tests import sim3_ransac_oracle as so

pytestmark = pytest.mark.gpu

ULP = float(np.finfo(np.float32).eps)
KEYS = ("R", "t", "s", "inlier", "hyp_inliers")


def run(cands, fix, min_inliers=so.MIN_INLIERS):
    from qsp_slam_amd.ba import sim3_ransac_batch
    return sim3_ransac_batch(cands, min_inliers, bool(fix), counts=True)


@pytest.fixture(scope="module")
def full():
    """the batch of 17, once per fix_scale setting"""
    return {fix: run(so.pool(fix), fix) for fix in (0, 1)}


@pytest.fixture(scope="module")
def every_flag():
    """per fix_scale setting and candidate: the flags (n_its, n) of every hypothesis, each evaluated as a candidate of its own"""
    out = {}
    for fix in (0, 1):
        singles, owner = [], []
        for i, c in enumerate(so.pool(fix)):
            for h in range(c["n_its"]):
                singles.append(dict(c, triples=c["triples"][h:h + 1], n_its=1))
                owner.append(i)
        res = run(singles, fix, min_inliers=-1)
        assert all(r["first_it"] == 1 for r in res)
        out[fix] = [np.array([r["inlier"] for r, o in zip(res, owner) if o == i], np.uint8).reshape(c["n_its"], len(c["X1c"]))
                    for i, c in enumerate(so.pool(fix))]
    return out


def same_bits(a, b):
    return (all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS) and a["first_it"] == b["first_it"]
            and a["n_inliers"] == b["n_inliers"])


@pytest.mark.parametrize("fix", [0, 1])
def test_flags_of_every_hypothesis(full, every_flag, fix):
    width = so.band()
    margins.within("sim3_ransac/band_f32_vs_f64", so.measured(), width)
    worst = 0.0
    for i, (c, r, g, fl) in enumerate(zip(so.pool(fix), so.pool_results(fix, "f64"), full[fix], every_flag[fix])):
        its = c["n_its"]
        assert np.array_equal(fl.sum(1), g["hyp_inliers"][:its]), i                     # the select kernel's bits are the count kernel's
        e = so.edge(r)[:its]
        diff = fl.astype(bool) != r["flags"][:its]
        if diff.any():
            worst = max(worst, float(e[diff].max()))
        print("fix_scale %d candidate %2d (%3d matches, %3d hypotheses): %d pairs differ from float64, largest knife-edge distance %.3e"
              % (fix, i, len(c["X1c"]), its, int(diff.sum()), float(e[diff].max()) if diff.any() else 0.0))
    print("fix_scale %d: largest knife-edge distance of a differing pair %.3e, BAND %.3e" % (fix, worst, width))
    # a pair may differ only strictly inside the band: `worst` is 0 when none differs, and then passes a band of 0 as well
    assert margins.within("sim3_ransac/fix%d/flag_edge" % fix, worst, width) and (worst < width or worst == 0.0)


@pytest.mark.parametrize("fix", [0, 1])
def test_counts_lie_in_the_oracles_interval(full, fix):
    width = so.band()
    for i, (c, r, g) in enumerate(zip(so.pool(fix), so.pool_results(fix, "f64"), full[fix])):
        its = c["n_its"]
        lo, hi = so.count_interval(r, width)
        n = g["hyp_inliers"]
        assert len(n) == len(c["triples"]) and (n[its:] == 0).all(), i
        assert ((lo[:its] <= n[:its]) & (n[:its] <= hi[:its])).all(), (i, n[:its], lo[:its], hi[:its])


@pytest.mark.parametrize("fix", [0, 1])
def test_first_success_and_transform(full, fix):
    worst = dict(R=0.0, t=0.0, s=0.0)
    n_success = 0
    for i, (c, r, g) in enumerate(zip(so.pool(fix), so.pool_results(fix, "f64"), full[fix])):
        first = so.first_success(r["count"], c["n_its"])
        assert g["first_it"] == first, (i, g["first_it"], first)
        assert g["inlier"].dtype == np.uint8 and len(g["inlier"]) == len(c["X1c"]) and g["n_inliers"] == int(g["inlier"].sum())
        if not first:
            assert g["n_inliers"] == 0 and not g["R"].any() and not g["t"].any() and g["s"] == 0
            continue
        n_success += 1
        h = first - 1
        assert g["n_inliers"] == g["hyp_inliers"][h] > so.MIN_INLIERS
        dist = so.flavour_distance(fix, i, h)                 # of THIS winner, not of the worst hypothesis of the pool
        scale = dict(R=1.0, t=max(1.0, float(np.abs(r["t"][h]).max())), s=max(1.0, float(r["s"][h])))
        for k in worst:
            err = float(np.abs(g[k].astype(np.float64) - r[k][h]).max())
            bar = max(4 * dist[k], 4 * ULP * scale[k])
            print("fix_scale %d candidate %2d %s: |gpu - float64| = %.3e, bar %.3e" % (fix, i, k, err, bar))
            assert margins.within("sim3_ransac/fix%d/c%02d/%s" % (fix, i, k), err, bar), (i, k, err, bar)
            worst[k] = max(worst[k], err)
        if fix:
            assert g["s"] == np.float32(1.0)                                                # exactly
    assert n_success >= 8
    print("fix_scale %d worst: %s" % (fix, worst))


@pytest.mark.parametrize("fix", [0, 1])
def test_alone_in_any_batch_at_any_position(full, fix):
    cands = so.pool(fix)
    for i, c in enumerate(cands):                                                            # batches of 1
        assert same_bits(run([c], fix)[0], full[fix][i]), i
    three = run([cands[i] for i in so.BATCH3], fix)                                          # a batch of 3, other neighbours
    for r, i in zip(three, so.BATCH3):
        assert same_bits(r, full[fix][i]), i
    rev = run(cands[::-1], fix)                                                              # every other position
    for r, g in zip(rev[::-1], full[fix]):
        assert same_bits(r, g)
    again = run(cands, fix)                                                                  # and a repeated run
    assert all(same_bits(a, b) for a, b in zip(again, full[fix]))


def test_nan_hypotheses_count_nothing(full):
    for fix in (0, 1):
        g = full[fix][11]
        # coincident, collinear.  The collinear triple (a line parallel to the optical axis) has N = diag(c, -c, -c, c): it counts 0
        # because the kernel's and the oracle's Jacobi both let the FIRST of equal eigenvalues win, e = (1,0,0,0), NaN.  With the
        # tie going to index 3 it would be a finite turn by pi.  This pins the library's tie-break, not cv::eigen's, whose choice in
        # a degenerate eigenspace is undefined.
        assert list(g["hyp_inliers"][:2]) == [0, 0]
        g = full[fix][12]
        assert g["first_it"] > 0 and g["inlier"][7] == 0 and g["inlier"][9] == 0             # z = 0 in either camera


def test_error_paths_leave_the_outputs_untouched():
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import sim3_ransac_batch
    assert sim3_ransac_batch([]) == []
    L = _lib.lib()
    cands = [so.pool(0)[i] for i in (7, 4)]
    n = [len(c["X1c"]) for c in cands]
    k = [len(c["triples"]) for c in cands]
    cat = lambda key, dt: np.ascontiguousarray(np.concatenate([np.asarray(c[key], dt).reshape(len(c[key]), -1) for c in cands]))
    K1, K2 = (np.ascontiguousarray(np.stack([c[key] for c in cands]), np.float32) for key in ("K1", "K2"))
    fl = [K1, K2, cat("X1c", np.float32), cat("X2c", np.float32), cat("sigma2_1", np.float32), cat("sigma2_2", np.float32)]
    good = dict(off=[0, n[0], n[0] + n[1]], its=[k[0], k[1]], toff=[0, k[0], k[0] + k[1]], tri=cat("triples", np.int32))
    first, ninl, hyp = np.full(2, -7, np.int32), np.full(2, -5, np.int32), np.full(sum(k), -3, np.int32)
    R, t, s, inl = np.full(18, 7.0, np.float32), np.full(6, 7.0, np.float32), np.full(2, 7.0, np.float32), np.full(sum(n), 9, np.uint8)

    def call(drop=None, n_cand=2, **kw):
        a = dict(good, **kw)
        ints = [_lib.i32ptr(np.ascontiguousarray(a[key], np.int32)) for key in ("off", "its", "toff", "tri")]
        f = [_lib.fptr(x) for x in fl]
        outs = [_lib.i32ptr(first), _lib.fptr(R), _lib.fptr(t), _lib.fptr(s), _lib.u8ptr(inl), _lib.i32ptr(ninl)]
        if drop is not None and drop < 4:
            ints[drop] = None
        elif drop is not None and drop < 10:
            f[drop - 4] = None
        elif drop is not None:
            outs[drop - 10] = None
        return L.qsp_sim3_ransac_batch(0, n_cand, *ints, *f, so.MIN_INLIERS, 0, *outs, _lib.i32ptr(hyp))

    untouched = lambda: ((first == -7).all() and (ninl == -5).all() and (hyp == -3).all() and (R == 7).all() and (t == 7).all()
                         and (s == 7).all() and (inl == 9).all())
    bad_tri = lambda row, v: np.concatenate([good["tri"][:row], np.array([v], np.int32), good["tri"][row + 1:]])
    refusals = [dict(off=[0, n[0], n[0] - 1]), dict(off=[1, n[0], n[0] + n[1]]), dict(off=[-1, n[0], n[0] + n[1]]),
                dict(toff=[0, k[0], k[0] - 1]), dict(toff=[1, k[0], k[0] + k[1]]),
                dict(its=[k[0] + 1, k[1]]), dict(its=[k[0], -1]),
                dict(tri=bad_tri(0, [0, 1, n[0]])), dict(tri=bad_tri(1, [-1, 1, 2])), dict(tri=bad_tri(k[0], [0, 1, n[1]])),
                dict(tri=bad_tri(2, [5, 5, 6])), dict(tri=bad_tri(3, [5, 6, 5])), dict(tri=bad_tri(k[0] + 1, [4, 6, 6]))]
    for kw in refusals:
        assert call(**kw) == _lib.QSP_ERR_INVALID and untouched(), kw
    # more than 1024 iterations, with the triples to go with them
    many = np.tile(np.array([[0, 1, 2]], np.int32), (1025, 1))
    assert call(its=[1025, k[1]], toff=[0, 1025, 1025 + k[1]], tri=np.concatenate([many, good["tri"][k[0]:]])) == _lib.QSP_ERR_INVALID
    assert untouched()
    for drop in range(16):
        assert call(drop) == _lib.QSP_ERR_INVALID and untouched(), drop
    assert call(n_cand=-1) == _lib.QSP_ERR_INVALID and untouched()
    assert call(n_cand=0) == _lib.QSP_OK and untouched()
    assert L.qsp_sim3_ransac_batch(0, 0, *([None] * 10), 20, 0, *([None] * 7)) == _lib.QSP_OK
    assert call() == _lib.QSP_OK and not untouched()
    r = so.pool_results(0, "f64")
    assert list(first) == [so.first_success(r[7]["count"], k[0]), so.first_success(r[4]["count"], k[1])]
