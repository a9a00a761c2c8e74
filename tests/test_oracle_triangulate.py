"""CPU: the conditions on the fixtures of tests/triangulate_oracle.py under which the GPU test can ask what it asks -- every branch
of the restatement is reached, every named mistake changes an output, the exact cases decide as stated, and almost no pair is
unstable under the reference's own rounding noise."""
import numpy as np
import pytest

from tests import triangulate_oracle as to


def test_every_branch_is_reached():
    """Over the fixtures together.  `w == 0` (:509, reason 3) cannot be reached with rotations for Rcw: an exact null vector (d, 0)
    of A means that d reprojects onto both key points, so the rays are parallel, cosParallaxRays is +-1 and the pair never enters
    the SVD branch.  The library takes any 3x3, though, and the `w_zero` fixture reaches it with a zero column in both."""
    total = {b: 0 for b in to.BRANCHES}
    for which in to.SCENES:
        for b, n in to.results(which)[1].items():
            total[b] += n
    print(total)
    assert [b for b, n in total.items() if n == 0] == []
    assert to.results("w_zero")[1]["w_zero"] == 2
    main = to.results("main")[1]
    # main alone reaches every reason but the two that need a constructed pose (3: w_zero; 8: the point ON a camera centre, in exact) ...
    reasons = np.bincount(np.concatenate([r["reason"] for r in to.results("main")[0]]), minlength=11)
    assert [int(c) for c in np.nonzero(reasons == 0)[0]] == [to.W_ZERO, to.DIST_ZERO]
    # ... and every path, with mono and stereo slots on both sides
    assert all(main[b] > 0 for b in ("svd", "svd_mono_mono", "unproject1", "unproject2", "low_parallax", "cos2_skipped_by_else", "mono1", "mono2",
                                     "stereo_err1", "stereo_err2", "accepted_not_first"))
    kf1, kf2s, _ = to.main_scene()
    assert len(kf1["u_right"]) == 300 and len({len(f["u_right"]) for f in kf2s}) == 3
    assert len({(float(f["fx"]), float(f["mb"]), len(f["scale_factors"])) for f in kf2s}) == 3


@pytest.mark.parametrize("mistake", to.MISTAKES)
def test_every_mistake_changes_an_output(mistake):
    where = dict(depth_lt="exact", chi_599="exact", chi_f32="exact", first_last="order").get(mistake, "main")
    wrong = to.triangulate(*to.scene(where), mistake=mistake)[0]
    right = to.results(where)[0]
    n = sum(int(np.any(a[k] != b[k])) for a, b in zip(wrong, right) for k in ("reason", "first", "accept"))
    assert n > 0, mistake


def test_the_exact_cases_decide_as_stated():
    kf1, kf2s, match, cases = to.exact_scene()
    res = to.results("exact")[0]
    rounds_up = rounds_down = 0
    for name, c in cases.items():
        k, i, want = c[:3]
        assert res[k]["reason"][i] == want, name
        assert res[k]["path"][i] in (to.PATH_UN1, to.PATH_UN2), name
        if len(c) == 4:                                    # sits one float32 step either side of chi * sigma2, evaluated in double
            e = res[k]["err2"][i, 0]
            assert e == c[3], name
            T = (7.8 if name.startswith("stereo") else 5.991) * float(kf1["sigma2"][i])
            assert (float(e) <= T) == ("below" in name) and abs(float(e) - T) <= float(np.spacing(e)), name
            if "above" in name:                            # where the float32 product rounds UP to this error, a float32 compare lets it pass
                up = float(np.float32(T)) > T
                rounds_up, rounds_down = rounds_up + up, rounds_down + (not up)
                assert (np.float32(e) > np.float32(T)) == (not up)
    assert rounds_up >= 2 and rounds_down >= 2
    assert res[cases["z1_zero"][0]]["z"][cases["z1_zero"][1], 0] == 0
    for name in ("ratio_low_equal", "ratio_low_above"):
        k, i, _ = cases[name]
        ro = kf1["scale"][i] / kf2s[k]["scale"][match[k, i]]
        lhs = res[k]["ratio_dist"][i] * kf1["ratio_factor"]
        assert (lhs == ro) == name.endswith("equal") and lhs <= ro
    for name in ("ratio_high_equal", "ratio_high_below"):
        k, i, _ = cases[name]
        ro = kf1["scale"][i] / kf2s[k]["scale"][match[k, i]]
        assert (res[k]["ratio_dist"][i] == ro * kf1["ratio_factor"]) == name.endswith("equal")
    k, i, _ = cases["dist_zero"]
    assert np.array_equal(res[k]["x3D"][i], kf2s[k]["Ow"]) and res[k]["z"][i, 1] > 0
    for name in ("depth0_kf1", "depth0_kf2"):
        k, i, _ = cases[name]
        assert (kf1["depth"][i] == 0 and kf1["u_right"][i] >= 0) or (kf2s[k]["depth"][match[k, i]] == 0 and kf2s[k]["u_right"][match[k, i]] >= 0)


@pytest.mark.parametrize("which", to.SCENES)
def test_the_unstable_share(which):
    """at most 2 % of the SVD-path pairs of a fixture may change their reason under a one-ulp perturbation; as built, none does,
    on or off the SVD path, in any fixture: the GPU test excepts nothing today"""
    res, nz = to.results(which)[0], to.noise_of(which)
    svd = np.concatenate([r["path"] == to.PATH_SVD for r in res])
    unstable = np.concatenate([n["unstable"] for n in nz])
    print("%s: %d SVD-path pairs, %d unstable; %d unstable elsewhere" % (which, svd.sum(), (unstable & svd).sum(), (unstable & ~svd).sum()))
    assert (unstable & svd).sum() <= 0.02 * svd.sum()
    assert not unstable.any()
    formed = np.concatenate([(r["path"] == to.PATH_SVD) & (r["reason"] != to.W_ZERO) for r in res])
    bar = np.concatenate([n["bar"] for n in nz])
    assert (bar[formed] > 0).all()                         # the formulation's noise is never nothing: a bar of 0 would ask for bit equality


def test_the_w_zero_pairs():
    res = to.results("w_zero")[0][0]
    assert list(res["reason"]) == [to.W_ZERO, to.W_ZERO] and list(res["path"]) == [to.PATH_SVD, to.PATH_SVD]
    assert not res["x3D"].any() and not res["z"].any() and (res["cos_rays"] > 0.5).all() and (res["cos_rays"] < 0.9998).all()
    kf1, kf2s, _ = to.w_zero_scene()
    assert not kf1["Rcw"][:, 0].any() and not kf2s[0]["Rcw"][:, 0].any() and kf1["u_right"][1] >= 0 and kf1["u_right"][0] < 0


def test_the_order_cases_and_the_edges():
    kf1, nbs, m, cases = to.order_scene()
    res = to.results("order")[0]
    acc = np.stack([r["accept"] for r in res])
    fst = np.stack([r["first"] for r in res])
    assert len(nbs) == 20
    for name, where in to.ORDER_CASES.items():
        i = cases[name]
        on = [] if where is None else list(where) if isinstance(where, tuple) else [where]
        assert list(np.nonzero(acc[:, i])[0]) == on, name
        assert list(np.nonzero(fst[:, i])[0]) == on[:1], name
    assert sorted(nc * n1 for nc, n1 in to.EDGE_COUNTS) == [0, 1, 63, 64, 65, 255, 256, 257, 513]
    for nc, n1 in to.EDGE_COUNTS:
        for at_last in (False, True):
            kf, nb, mm = to.edge_scene(nc, n1, at_last)
            r, _ = to.triangulate(kf, nb, mm)
            if nc * n1:
                assert sum(x["n_new"] for x in r) == 1 and r[-1 if at_last else 0]["first"][-1 if at_last else 0]
                assert not to.noise(kf, nb, mm)[-1 if at_last else 0]["unstable"].any()
