"""CPU: the numpy restatement of the object map-point gate (tests/object_gate_oracle.py) against hand-built cases, and the
fixtures of the GPU test against the two flavours of the restatement: outside the knife-edge band float32 and double arithmetic
set the same flags, so a disagreement of the device with the double flavour there is the device's."""
import numpy as np
import pytest

from tests import object_gate_cases as GC
from tests import object_gate_oracle as GO


def test_order_statistic_is_what_sort_leaves():
    rng = np.random.default_rng(0)
    for n in (1, 2, 19, 20, 21, 300):
        for x in (rng.normal(size=n).astype(np.float32), np.round(rng.normal(size=n) * 2).astype(np.float32)):   # the second: ties
            s = np.sort(x)
            for k in sorted({0, int(0.05 * n), int(0.95 * n), n - 1}):
                assert GO.order_statistic(x, k) == s[k]


def _box_cloud():
    """a 21 x 11 x 15 lattice filling [-1, 1] x [-0.25, 0.25] x [-0.6, 0.6] about (3, -2, 5): the axes are the principal axes by
    construction (largest extent x, smallest y), plus two points far outside the box and one more than 1 m from the mean"""
    g = np.stack(np.meshgrid(np.linspace(-1, 1, 21), np.linspace(-0.25, 0.25, 11), np.linspace(-0.6, 0.6, 15), indexing="ij"), -1)
    x = g.reshape(-1, 3)
    x = x[np.linalg.norm(x, axis=1) < 0.999]                     # nothing of the lattice is erased
    extra = np.array([[0.0, 0.9, 0.0], [0.0, 0.0, -0.95], [0.0, 1.8, 0.0]])
    return np.concatenate([x, extra]) + np.array([3.0, -2.0, 5.0]), len(x)


@pytest.mark.parametrize("flavour", ["f32", "f64"])
def test_axis_aligned_box_cloud(flavour):
    x, n_lat = _box_cloud()
    r = GO.pca_gate(x, flavour)
    assert r["status"] == GO.OK
    assert list(np.nonzero(r["erased"])[0]) == [n_lat + 2]
    # principal axes: x largest, y smallest -> R = [v1 | v0 | -v2] = [+-z | +-y | +-x] with the y column pointing down
    R = r["R"]
    assert np.allclose(np.abs(R), [[0, 0, 1], [0, 1, 0], [1, 0, 0]], atol=1e-5)
    assert R[1, 1] < 0 and np.linalg.det(R) > 0
    X = x[~r["erased"]]
    n = len(X)
    lo, hi = int(0.05 * n), int(0.95 * n)
    s = np.sort(X.astype(np.float32).astype(np.float64), axis=0)
    ext = s[hi] - s[lo]
    assert np.allclose(r["whl"], [ext[2], ext[1], ext[0]], atol=1e-5)          # w along world z, h along y, l along x
    assert np.allclose(r["centre_w"], (s[hi] + s[lo]) / 2, atol=1e-5)
    assert np.allclose(r["T_wo"][:3, :3], 0.40 * ext[0] * R, atol=1e-5) and np.allclose(r["T_wo"][:3, 3], r["centre_w"], atol=1e-6)
    d = np.abs(X - (s[hi] + s[lo]) / 2)
    expect = (d > 1.2 * ext / 2 + 1e-4).any(axis=1)
    assert np.array_equal(r["outlier"][~r["erased"]], expect)
    assert r["outlier"][n_lat] and r["outlier"][n_lat + 1] and not r["outlier"][n_lat + 2]


def test_model_gate_by_hand():
    m = GC.model_cases()["six_planes"]
    for flavour in ("f32", "f64"):
        r = GO.model_gate(m["pts_world"], m["T_wo"], m["vertices"], flavour)
        assert r["status"] == GO.OK and np.array_equal(r["outlier"], m["expect"]) and not r["erased"].any()
        v = np.asarray(m["vertices"], np.float32)
        assert np.allclose(r["whl"], (v.max(axis=0) - v.min(axis=0)) * 1.7, rtol=1e-5)
    assert GO.model_gate(m["pts_world"], m["T_wo"], m["vertices"][:10])["status"] == GO.SKIPPED
    assert GO.model_gate(m["pts_world"], m["T_wo"], None)["status"] == GO.SKIPPED


def test_ymin_positive_separates_the_two_readings():
    """factors on the coordinates (the reference) against factors on the extent about the centre: different flags"""
    c = GC.model_cases()["ymin_positive"]
    r = GO.gate(c)
    v = np.asarray(c["vertices"], np.float32).astype(np.float64)
    assert v[:, 1].min() > 0
    T = c["T_wo"].astype(np.float64)
    xo = (c["pts_world"].astype(np.float64) - T[:3, 3]) @ np.linalg.inv(T[:3, :3]).T
    mid, half = (v.max(axis=0) + v.min(axis=0)) / 2, (v.max(axis=0) - v.min(axis=0)) / 2
    other = (np.abs(xo - mid) > np.array([1.2, 1.5, 1.2]) * half).any(axis=1)
    assert np.count_nonzero(other != r["outlier"]) > 20


def _all_cases():
    c = dict(GC.pca_cases())
    c.update(GC.model_cases())
    return c        # (not coplanar3: its box has no thickness, every point sits on a face; the GPU test checks no flag of it)


def test_fixtures_keep_float32_and_double_apart_only_inside_the_band():
    """f32 and f64 agree on every flag of every fixture outside the band, and the band holds at most max(1, 0.5 %) of an
    object's points: the cap of the GPU test is left to the reference's own arithmetic alone"""
    for name, c in _all_cases().items():
        a, b = GO.gate(c, "f32"), GO.gate(c, "f64")
        assert a["status"] == b["status"], name
        out = b["edge"] >= GC.BAND
        n = len(out)
        assert np.count_nonzero(~out) <= max(1, int(0.005 * n)), (name, np.count_nonzero(~out))
        assert np.array_equal(a["erased"][out], b["erased"][out]), name
        assert np.array_equal(a["outlier"][out], b["outlier"][out]), name
        if b["status"] == GO.OK and "vertices" not in c:
            scale = np.abs(c["pts_world"]).max()
            flip = np.diag([-1.0, 1.0, -1.0])
            assert min(np.abs(a["R"] - b["R"]).max(), np.abs(a["R"] @ flip - b["R"]).max()) < 1e-4, name
            assert np.abs(a["whl"] - b["whl"]).max() < 1e-5 * max(scale, 1), name
            assert np.abs(a["centre_w"] - b["centre_w"]).max() < 1e-5 * max(scale, 1), name
