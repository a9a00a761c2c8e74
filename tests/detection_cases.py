"""The cases of the detection-marshalling edge tests (qsp_refine_detections, csrc/detections.hpp), built by post-processing
synth.make_detections and shared by tests/test_oracle_detections.py (CPU: the fixture conditions) and tests/test_gpu_detections.py.

  * with_intrinsics: a detection seen through another camera -- K replaced, the key-point pixels moved so that the rays still hit
    the object.  synth.make_detections forms px = (fx * ray_x + cx, fy * ray_y + cy) in float64 from one K for every detection; the
    rays are taken back out of its pixels with that K and pushed through the new one, in float64, then cast to float32.
  * with_yaw(det, k, flips): Sim3Two's rotation block right-multiplied by a rotation about e_y of -k * 2 pi / flips, so that flip
    hypothesis k (which multiplies by +k * 2 pi / flips, src/LocalMapping_util.cc:722-726) lands on the perturbed ground truth and
    hypothesis 0 starts k flips away from it.
  * with_counts: a detection cut or grown to given numbers of map points, feature points and background rays.  Grown arrays repeat
    the detection's own rows with a seeded jitter, so that no two rows are equal (a copy from the wrong index shows) and the
    observations stay on the object.
  * MIDDLE_FLIP: seeds chosen with the oracle alone, on the CPU, until the condition stated at `middle_flip_holds` holds;
    tests/test_oracle_detections.py asserts it.

No fixture here has hypotheses of one detection that differ in `alive` by a margin.  The flags can differ through the render term's
sample count (fewer than 10 samples in the unit ball, loss.py:73) or through its kept rows (none: optimizer.py:193-194).  A search
with the oracle over 204 seeds (1 to 3 feature rays, 2 to 6 background rays, 8 to 20 points, 3 and 4 iterations, four flips, the
first hypothesis turned 1 to 3 flips off the truth) found 49 detections whose first hypothesis ends not good and a later one good,
every one of them through the kept rows: a ray that meets the object crosses the ball near its centre, and the smallest count any
hypothesis saw at any iteration was 23.  A row count has no margin that float32 against the oracle cannot move, so none was made
a fixture; detection 1 of test_c_abi_optional_arguments happens to be such a case and is held to the serial calls like the rest.

CPU only: numpy, the oracles and the synthetic-scene generator."""
import functools
import math
import os

import numpy as np

from oracle import detections_oracle as DO
from oracle import sdf_oracle as so
from qsp_slam_amd import synth
from tests.sim3_oracle import CAM_A, CAM_B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32

# fx fy cx cy: fx != fy, all principal points distinct.  The first two are the cameras of tests/sim3_oracle.py (TUM fr1 / fr2 as
# ORB-SLAM2's example settings give them); the other two are made up in the range of the public EuRoC and KITTI calibrations.
INTRINSICS = (np.asarray(CAM_A, np.float64), np.asarray(CAM_B, np.float64),
              np.array([458.7, 457.3, 367.2, 248.4]), np.array([718.9, 707.1, 607.2, 185.2]))

LOSS_GAP = 1e-2                 # the kept middle flip's loss is below every other good one's by this, relative (oracle vs GPU loss: decoder tolerance)


def with_intrinsics(det, K):
    K0 = np.asarray(det["K"], np.float64)
    K = np.asarray(K, np.float64).reshape(4)
    px = np.asarray(det["fg_px"], np.float64).reshape(-1, 2)
    ray = np.stack([(px[:, 0] - K0[2]) / K0[0], (px[:, 1] - K0[3]) / K0[1]], axis=1)
    out = dict(det)
    out["K"] = K.astype(F)
    out["fg_px"] = np.stack([K[0] * ray[:, 0] + K[2], K[1] * ray[:, 1] + K[3]], axis=1).astype(F)
    return out


def with_yaw(det, k, flips):
    out = dict(det)
    T = np.asarray(det["T_wo"], np.float64).copy()
    T[:3, :3] = T[:3, :3] @ synth.rot_y(-k * 2.0 * math.pi / flips)
    out["T_wo"] = T.astype(F)
    return out


def _grown(a, n, rng, jitter):
    """n rows of `a`: its first n, or all of them followed by repeats that a seeded normal jitter (per column) makes distinct"""
    a = np.asarray(a, F)
    m = a.shape[0]
    if n <= m:
        return a[:n].copy()
    idx = np.arange(n - m) % m
    extra = a[idx].astype(np.float64) + rng.normal(size=(n - m, a.shape[1])) * np.asarray(jitter, np.float64)
    return np.concatenate([a, extra.astype(F)], axis=0)


def with_counts(det, n_pts=None, n_fg=None, n_bg=None, seed=0):
    """`det` with n_pts map points, n_fg feature points and n_bg background rays (None: as it is).  Jitter: 1 mm on world
    positions, 0.5 px on pixels, 1e-4 on the x and y of a background ray (its z stays 1)."""
    rng = np.random.default_rng(4000 + seed)
    out = dict(det)
    if n_pts is not None:
        out["pts_world"] = _grown(det["pts_world"], n_pts, rng, 1e-3)
    if n_fg is not None:
        out["fg_world"] = _grown(det["fg_world"], n_fg, rng, 1e-3)
        out["fg_px"] = _grown(det["fg_px"], n_fg, rng, 0.5)
    if n_bg is not None:
        out["bg_rays"] = _grown(det["bg_rays"], n_bg, rng, (1e-4, 1e-4, 0.0))
    return out


# ---- the stride cases: one k_det_assemble launch is min(64, ceil(max_items / 256)) blocks of 256 threads per detection, so
# ---- 16384 threads at most; item 16384 of a loop is the first one of its second pass
ONE_PASS = 64 * 256
TINY = dict(n_pts=37, n_fg=12, n_bg=4)          # 16 rays: runs under gx = 64 beside the large ones


def stride_detections():
    """ONE call: [tiny, 16385 points, 16385 feature points, 5462 background rays (16386 floats), exactly 16384 points, tiny].  The
    large ones are refined as a single hypothesis (found_good_orientation), the tiny ones with all flips."""
    base = synth.make_detections(41, 6, 300, n_fg=48, n_bg=16, n_kf=2)
    dets = [with_counts(base[0], **TINY),
            with_counts(base[1], n_pts=ONE_PASS + 1, n_fg=12, n_bg=4, seed=1),
            with_counts(base[2], n_pts=64, n_fg=ONE_PASS + 1, n_bg=8, seed=2),
            with_counts(base[3], n_pts=64, n_fg=24, n_bg=5462, seed=3),
            with_counts(base[4], n_pts=ONE_PASS, n_fg=12, n_bg=4, seed=4),
            with_counts(base[5], **TINY)]
    for d in dets[1:5]:
        d["found_good_orientation"] = True
    return dets


# ---- oracle runs of a detection's hypotheses ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_decoder():
    return so.load_decoder_npz(os.path.join(GOLDEN, "decoder_8x512.npz"))


def in_ball_count(cfg, T_oc, rays):
    """the number of ray samples in the unit ball that gn_iteration's render term sees from the state T_oc (loss.py:60-74)"""
    T_oc = np.asarray(T_oc, F)
    T_co = np.linalg.inv(T_oc).astype(F)
    scale = F(np.linalg.det(T_co[:3, :3])) ** F(1.0 / 3.0)
    depths = np.linspace(T_co[2, 3] - scale, T_co[2, 3] + scale, cfg.n_depth, dtype=F)
    p = so.transform_points(T_oc, np.asarray(rays, F)[:, None, :] * depths[:, None])
    return int((np.sqrt((p * p).sum(-1, dtype=F)) < 1.0).sum())


def oracle_hypotheses(det, flips, n_iter):
    """Optimizer.reconstruct_object of the oracle on the oracle-assembled inputs, for every flip hypothesis: a list of
    dict(is_good, loss, fail, counts, K) -- counts[e] the in-ball sample count iteration e saw, K[e] its kept render rows"""
    dec, cfg = oracle_decoder(), so.JointConfig(n_iter=n_iter)
    pts, rays, depth = DO.assemble(det)
    n_fg = depth.shape[0]
    dobs = np.concatenate([depth, np.zeros(rays.shape[0] - n_fg, F)])
    nf = 1 if det.get("found_good_orientation") else flips
    out = []
    for T0 in DO.init_poses(det, nf, 2.0 * math.pi / flips):
        T_oc = np.linalg.inv(T0).astype(F)
        z = np.zeros(64, F) if det.get("code") is None else np.asarray(det["code"], F).copy()
        h = dict(is_good=True, loss=0.0, fail=None, counts=[], K=[])
        for _ in range(n_iter):
            h["counts"].append(in_ball_count(cfg, T_oc, rays))
            it = so.gn_iteration(dec, cfg, T_oc, z, pts, rays, dobs, n_fg)
            if it["fail"] is not None:
                h["is_good"], h["fail"] = False, it["fail"]
                break
            h["K"].append(it["K"])
            h["loss"] = it["loss"]
            T_oc, z = it["T_oc_new"], it["code_new"]
        out.append(h)
    return out


# ---- a middle flip kept because its loss is smaller ---------------------------------------------------------------------------
# name: (flips, n_iter, seed, sizes, yaw k per detection -- None: untouched)
MIDDLE_FLIP = {
    "flips4": (4, 2, 9, dict(n_pts=150, n_fg=40, n_bg=16), (1, 2, 3, None)),
    "flips6": (6, 2, 1, dict(n_pts=150, n_fg=40, n_bg=16), (3,)),
}


def middle_flip_detections(name):
    flips, n_iter, seed, sizes, yaws = MIDDLE_FLIP[name]
    dets = synth.make_detections(seed, len(yaws), sizes["n_pts"], n_fg=sizes["n_fg"], n_bg=sizes["n_bg"], n_kf=2)
    return [d if k is None else with_yaw(d, k, flips) for d, k in zip(dets, yaws)]


def middle_flip_holds(hyps, k):
    """hypothesis k good, and its loss at least LOSS_GAP (relative) below the loss of every other good hypothesis"""
    if not hyps[k]["is_good"]:
        return False
    return all(hyps[k]["loss"] <= (1.0 - LOSS_GAP) * h["loss"] for j, h in enumerate(hyps) if j != k and h["is_good"])
