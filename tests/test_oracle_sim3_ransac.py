"""CPU: tests/sim3_ransac_oracle.py, the restatement of Sim3Solver that qsp_sim3_ransac_batch is held to, checked against what it
must do on its own, the two helpers of qsp_slam_amd.ba that feed the call, and the conditions on the fixtures that keep the
undecided band of tests/test_gpu_sim3_ransac.py from hiding a failure."""
import numpy as np
import pytest

from tests import sim3_ransac_oracle as so


@pytest.mark.parametrize("flavour", ["f32", "f64"])
@pytest.mark.parametrize("fix", [0, 1])
def test_a_planted_sim3_is_recovered(fix, flavour):
    """noise and three outliers in ten: the first success is near the planted transform and finds most of the related pairs"""
    c = so.pool(fix)[8]
    r = so.pool_results(fix, flavour)[8]
    first = so.first_success(r["count"], c["n_its"])
    assert first > 0
    h, true = first - 1, c["true"]
    assert r["count"][h] > so.MIN_INLIERS and r["count"][h] == r["flags"][h].sum()
    assert np.abs(r["R"][h] - true["R"]).max() < 0.02 and np.abs(r["t"][h] - true["t"]).max() < 0.1 and abs(r["s"][h] - true["s"]) < 0.02
    best = int(np.argmax(r["count"]))
    assert r["count"][best] > 0.5 * len(c["X1c"])
    assert np.abs(r["R"][best] - true["R"]).max() < 0.01 and abs(r["s"][best] - true["s"]) < 0.01
    if fix:
        assert (r["s"] == 1).all()


@pytest.mark.parametrize("fix", [0, 1])
def test_first_success_is_the_serial_loop(fix):
    """the min-reduction argument: the literal loop with its `>= best` bookkeeping returns the first index above minInliers, on the
    fixtures' counts and on random count sequences with ties, rises and falls around minInliers"""
    for c, r in zip(so.pool(fix), so.pool_results(fix, "f64")):
        assert so.serial_loop(r["count"], c["n_its"]) == so.first_success(r["count"], c["n_its"])
    rng = np.random.default_rng(5)
    hits = 0
    for _ in range(300):
        count = rng.integers(0, 26, int(rng.integers(0, 40)))
        assert so.serial_loop(count, len(count)) == so.first_success(count, len(count))
        hits += so.first_success(count, len(count)) > 0
    assert 50 < hits < 300


def test_iteration_formula():
    from qsp_slam_amd.ba import sim3_ransac_iterations
    # N = 20: the `==` branch; 21: ceil(log .01 / log(1 - (20/21)^3)) = ceil(2.31) = 3; 40: eps = .5, ceil(34.49) = 35; 100, 300: capped
    assert [sim3_ransac_iterations(n) for n in (20, 21, 40, 100, 300)] == [1, 3, 35, 300, 300]
    for n in (20, 21, 40, 63, 64, 65, 100, 129, 300):
        assert sim3_ransac_iterations(n) == so.iterations(n)
    assert sim3_ransac_iterations(19) == 0 and sim3_ransac_iterations(0) == 0            # iterate() bails, :146-150
    assert sim3_ransac_iterations(40, max_its=10) == 10 and sim3_ransac_iterations(30, min_inliers=30) == 1


def test_draw_triples_never_repeats_an_index():
    from qsp_slam_amd.ba import draw_triples
    rng = np.random.default_rng(3)
    for n in (3, 4, 20, 65):
        t = draw_triples(n, 200, rng)
        assert t.shape == (200, 3) and t.dtype == np.int32 and t.min() >= 0 and t.max() < n
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    assert len(np.unique(draw_triples(20, 200, rng), axis=0)) > 150                       # and it does draw
    assert sorted(draw_triples(3, 1, rng)[0]) == [0, 1, 2]
    # swap-with-back: with every draw 0 the list 0 1 2 3 4 gives 0, then 4 (moved to the front), then 3
    class Zero(object):
        def integers(self, lo, hi):
            return 0
    assert list(draw_triples(5, 1, Zero())[0]) == [0, 4, 3]


@pytest.mark.parametrize("flavour", ["f32", "f64"])
@pytest.mark.parametrize("fix", [0, 1])
def test_degenerate_triples_count_nothing(fix, flavour):
    r = so.pool_results(fix, flavour)[11]
    assert so.pool(fix)[11]["kind"] == "degenerate"
    for h in (0, 1):                                         # coincident, collinear
        assert r["count"][h] == 0 and not r["flags"][h].any()
        assert np.isnan(r["T12"][h]).all()
    assert np.isfinite(r["T12"][2:]).all()
    z = so.pool_results(fix, flavour)[12]                    # z = 0: matches 7 and 9 are outliers under every hypothesis
    assert not z["flags"][:, 7].any() and not z["flags"][:, 9].any() and np.isfinite(z["T12"]).all()


def test_the_fixtures_cover_what_the_gpu_test_says_they_do():
    for fix in (0, 1):
        cands, res = so.pool(fix), so.pool_results(fix, "f64")
        assert len(cands) == 17
        assert {len(c["X1c"]) for c in cands} >= {0, 3, 19, 20, 21, 63, 64, 65, 129, 300}
        its = [c["n_its"] for c in cands]
        assert {0, 1, 5, 6} <= set(its) and any(c["n_its"] == so.iterations(len(c["X1c"])) and c["n_its"] > 6 for c in cands)
        assert any(c["n_its"] < len(c["triples"]) for c in cands)
        first = [so.first_success(r["count"], c["n_its"]) for c, r in zip(cands, res)]
        assert first[10] == 0 and cands[10]["kind"] == "outliers" and cands[10]["n_its"] == 300
        assert first[4] == 1 and first[3] == 0                                            # 21 exact pairs: at once; 20: never
        assert any(f > 1 for f in first)
        for c in cands:                                                                   # what the library refuses is not in here
            t, n = c["triples"], len(c["X1c"])
            assert len(t) == 0 or (t.min() >= 0 and t.max() < n and (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all()
                                   and (t[:, 0] != t[:, 2]).all())


def test_the_band_cannot_hide_a_failure():
    """BAND = 4 x the smallest band outside which the float32 flavour agrees with float64 on every fixture.  Inside it the GPU test
    decides nothing, so: at most max(1, 0.5 %) of a candidate's pairs lie inside, and no hypothesis up to the first success has a
    count interval that straddles minInliers -- the first success is decided outside the band.

    On the present fixtures the two flavours agree on every pair, the measured band is 0, BAND is 0 and the GPU test holds the
    flags to equality (which then rests on the device's atan2 / sin / cos keeping every decision as well).  With a band of 0
    nothing lies inside it and both conditions below hold trivially; they decide something again as soon as a change of the
    fixtures or of the restatement makes the measured band positive."""
    width = so.band()
    print("measured band %.3e  BAND %.3e" % (so.measured(), width))
    assert np.isfinite(width) and width < 0.05
    for fix in (0, 1):
        for i, (c, r) in enumerate(zip(so.pool(fix), so.pool_results(fix, "f64"))):
            its = c["n_its"]
            frac, num = so.in_band_fraction(r, its, width)
            assert num <= max(1, 0.005 * its * len(c["X1c"])), (fix, i, num, frac)
            first = so.first_success(r["count"], its)
            lo, hi = so.count_interval(r, width)
            upto = first if first else its
            assert not ((lo[:upto] <= so.MIN_INLIERS) & (hi[:upto] > so.MIN_INLIERS)).any(), (fix, i)
