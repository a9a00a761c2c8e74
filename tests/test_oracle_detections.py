"""CPU: the marshalling restatement (oracle/detections_oracle.py) against float64 closed forms and the keep rule against the
host-side selection of the Python mirror (reference src/LocalMapping_util.cc:585-760)."""
import math

import numpy as np
import pytest

from oracle import detections_oracle as DO
from qsp_slam_amd import synth


def test_assemble_matches_float64_closed_form():
    dets = synth.make_detections(3, 4, 500, n_fg=64, n_bg=32)
    for d in dets:
        pts, rays, depth = DO.assemble(d)
        T = d["T_cw"].astype(np.float64)
        ref = (T[:3, :3] @ d["pts_world"].astype(np.float64).T).T + T[:3, 3]
        assert pts.dtype == np.float32 and np.abs(pts - ref).max() < 2e-6 * max(1.0, np.abs(ref).max())
        fx, fy, cx, cy = d["K"].astype(np.float64)
        px = d["fg_px"].astype(np.float64)
        fg = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(len(px))], axis=1)
        n_f = len(px)
        assert rays.shape == (n_f + len(d["bg_rays"]), 3)
        assert np.abs(rays[:n_f] - fg).max() < 1e-6                # tolerance: float32 rounding of 3 products
        assert np.array_equal(rays[n_f:], d["bg_rays"])
        zref = ((T[:3, :3] @ d["fg_world"].astype(np.float64).T).T + T[:3, 3])[:, 2]
        assert np.abs(depth - zref).max() < 2e-6 * np.abs(zref).max()
        # the synthetic scene is consistent: the assembled views reproduce what make_object_views generated
        assert np.abs(rays[:n_f, :2] * depth[:, None] - (fg * zref[:, None])[:, :2]).max() < 1e-4


def test_eigen_inverse_of_intrinsics():
    K4 = np.array([535.4, 539.2, 320.1, 247.6], np.float32)
    inv = DO.eigen_inverse_k(K4)
    Km = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], np.float64)
    assert np.abs(inv.astype(np.float64) @ Km - np.eye(3)).max() < 1e-6
    assert inv[1, 0] == 0 and inv[2, 0] == 0 and inv[2, 1] == 0 and inv[0, 1] == 0


def test_flip_poses():
    d = synth.make_detections(5, 1, 100, n_fg=16, n_bg=8)[0]
    ang = 2 * math.pi / 4
    T = DO.init_poses(d, 4, ang)
    T_cw, T_wo = d["T_cw"].astype(np.float64), d["T_wo"].astype(np.float64)
    assert np.abs(T[0] - T_cw @ T_wo).max() < 1e-5
    for k in range(1, 4):
        c, s = math.cos(k * ang), math.sin(k * ang)
        Fm = T_wo.copy()
        Fm[:3, :3] = T_wo[:3, :3] @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        assert np.abs(T[k] - T_cw @ Fm).max() < 1e-5
    R = DO.rot_y(2, ang)                          # float(pi): cosf = -1, sinf = -8.7e-8 (not 0)
    assert R[0, 0] == np.float32(-1.0) and R[1, 1] == np.float32(1.0) and abs(R[0, 2]) < 1e-6 and R[2, 0] == -R[0, 2]


def test_keep_rule_cases():
    # first good, later smaller and good -> replaced; later smaller but bad -> kept
    assert DO.keep_rule([True, True, True, True], [3.0, 2.0, 2.5, 1.0]) == 3
    assert DO.keep_rule([True, False, True, True], [3.0, 1.0, 3.5, 3.0]) == 0      # 3.0 > 3.0 is false
    assert DO.keep_rule([False, False, True, True], [1.0, 9.0, 5.0, 6.0]) == 2     # a bad holder is always replaced ...
    assert DO.keep_rule([False, False, False, False], [1.0, 2.0, 3.0, 4.0]) == 3   # ... even by another bad one
    assert DO.keep_rule([True, True], [float("nan"), 1.0]) == 0                    # NaN compares false
    assert DO.keep_rule([True], [1.0]) == 0
    # same rule as the host-side selection of reconstruct_objects_batched (qsp_slam_amd/reconstruct/optimizer.py)
    rng = np.random.default_rng(0)
    for _ in range(200):
        good = rng.random(4) < 0.6
        loss = rng.choice([0.5, 1.0, 1.0, 2.0, float("nan")], size=4)
        best = 0
        for k in range(1, 4):
            if (not good[best]) or (good[k] and loss[k] < loss[best]):
                best = k
        assert DO.keep_rule(list(good), list(loss)) == best


# ---- the fixture conditions of tests/detection_cases.py (the GPU side: tests/test_gpu_detections.py) ---------------------------

def test_distinct_intrinsics_give_distinct_inverses_and_rays_that_still_hit_the_object():
    from tests import detection_cases as dc
    Ks = [np.asarray(K, np.float32) for K in dc.INTRINSICS]
    assert all(K[0] != K[1] for K in Ks)
    for col in range(4):
        assert len({float(K[col]) for K in Ks}) == 4
    inv = [DO.eigen_inverse_k(K) for K in Ks]
    for i in range(4):
        for j in range(i):
            # every entry the rays use differs between any two cameras: a kernel reading another detection's K shows in x and in y
            assert all(inv[i][r, c] != inv[j][r, c] for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)))
    base = synth.make_detections(11, 4, 700, n_fg=96, n_bg=40, n_kf=2)
    for d, K in zip(base, Ks):
        e = dc.with_intrinsics(d, K)
        assert e["K"].dtype == np.float32 and e["fg_px"].dtype == np.float32 and e["fg_px"].shape == d["fg_px"].shape
        r0, r1 = DO.assemble(d)[1], DO.assemble(e)[1]
        assert np.abs(r1 - r0).max() < 2e-6                 # the same rays (float32 pixels of ~600: 3e-5 px / fx each way)
        if not np.array_equal(K, d["K"]):
            wrong = DO.assemble(dict(e, K=d["K"]))[1]
            assert np.abs(wrong - r0)[:96].max() > 1e-2     # and the pixels did move: the old K no longer fits them


def test_with_yaw_puts_flip_k_on_the_perturbed_ground_truth():
    from tests import detection_cases as dc
    d = synth.make_detections(5, 1, 100, n_fg=16, n_bg=8)[0]
    for flips, k in ((4, 1), (4, 2), (4, 3), (6, 3)):
        e = dc.with_yaw(d, k, flips)
        T = DO.init_poses(e, flips, 2 * math.pi / flips)
        T0 = DO.init_poses(d, 1, 2 * math.pi / flips)[0]
        assert np.abs(T[k] - T0).max() < 1e-5
        assert all(np.abs(T[j] - T0).max() > 0.1 for j in range(flips) if j != k)
        assert np.array_equal(e["T_wo"][:, 3], d["T_wo"][:, 3])


def test_with_counts_and_the_stride_cases():
    from tests import detection_cases as dc
    dets = dc.stride_detections()
    assert [len(d["pts_world"]) for d in dets] == [37, dc.ONE_PASS + 1, 64, 64, dc.ONE_PASS, 37]
    assert [len(d["fg_px"]) for d in dets] == [12, 12, dc.ONE_PASS + 1, 24, 12, 12]
    assert [3 * len(d["bg_rays"]) for d in dets] == [12, 12, 24, dc.ONE_PASS + 2, 12, 12]
    for d in dets:
        assert len(d["fg_world"]) == len(d["fg_px"])
        for key in ("pts_world", "fg_px", "fg_world", "bg_rays"):
            assert d[key].dtype == np.float32 and len(np.unique(d[key], axis=0)) == len(d[key]), key      # no two rows equal
        assert np.all(d["bg_rays"][:, 2] == 1.0)
    # grown observations stay on the object: their rays meet their map points to a centimetre
    big = dets[2]
    pts, rays, depth = DO.assemble(big)
    assert np.abs(rays[:dc.ONE_PASS + 1, :2] * depth[:, None] - DO.cv_affine(big["T_cw"], big["fg_world"])[:, :2]).max() < 2e-2



@pytest.mark.parametrize("name", ["flips4", "flips6"])
def test_middle_flip_fixtures_keep_flip_k_by_a_loss_gap(name):
    """under the oracle alone: hypothesis k good, its loss at least 1e-2 (relative) below every other good hypothesis's"""
    from tests import detection_cases as dc
    flips, n_iter, _, _, yaws = dc.MIDDLE_FLIP[name]
    kept = []
    for d, k in zip(dc.middle_flip_detections(name), yaws):
        k = k or 0
        hyps = dc.oracle_hypotheses(d, flips, n_iter)
        assert dc.middle_flip_holds(hyps, k), (name, k, [(h["is_good"], h["loss"]) for h in hyps])
        assert DO.keep_rule([h["is_good"] for h in hyps], [h["loss"] for h in hyps]) == k
        # the two-outcome rule a wrong kernel could follow ("first if good, else last") keeps another one
        assert k == 0 or hyps[0]["is_good"]
        kept.append(k)
    assert any(0 < k < flips - 1 for k in kept)


def test_fixture_predicates():
    from tests import detection_cases as dc
    h = lambda good, loss=1.0: dict(is_good=good, loss=loss)
    assert dc.middle_flip_holds([h(True, 1.0), h(True, 0.98), h(False, 0.1)], 1)
    assert not dc.middle_flip_holds([h(True, 1.0), h(True, 0.995)], 1)
    assert not dc.middle_flip_holds([h(True, 1.0), h(False, 0.5)], 1)
