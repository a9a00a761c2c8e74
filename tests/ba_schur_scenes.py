"""The three forms in which a Levenberg-Marquardt trial of the bundle adjustment builds the reduced camera system (the trial loop of
qsp_ba_optimize, csrc/ba_solver.hip), one scene per regime, each the smallest that reaches it.  Shared by
tests/test_oracle_ba_schur.py (the C oracle on the CPU: is every scene what the table says, and is the reference sharp there?) and
tests/test_gpu_ba_schur.py (the device against that oracle, with qsp_ba_stats.schur_form as the witness of what ran).  Nothing here
touches a GPU.

    form 0  pair lists     k_trial_stage1 + k_schur_pairs                    the mode is `deterministic`: the default whenever
                                                                             sum_l k_l (k_l + 1) / 2 <= PAIR_CAP and n_kf^2 <= 2^24
    form 1  per landmark   k_schur_prepare + k_schur_points                  atomic mode, and n_edge < ROWS_MIN_EDGES or the row
                                                                             block 8 (6 dimp + 6) bytes does not fit LDS_MAX
    form 2  block rows     k_schur_prepare + k_schur_dinv + k_schur_rows     atomic mode otherwise
    form -1 no reduced system: no free key-frame or object (dimp == 0), or no trial ran

`predict()` restates that rule from counts alone.  dimp is the dense dimension padded to 64: 6 x free key-frames with the objects
eliminated in front of the solve, 6 x (free key-frames + active objects) with the objects inside; the elimination is dropped when a
6 x dimp row block of the key-frames alone exceeds LDS_MAX (k_obj_rows).  The linearisation and k_schur_rows cut each key-frame's
edges into pieces of KSPLIT_SMALL edges below KSPLIT_SMALL_BELOW edges and KSPLIT from there on.

Every scene has at least one fixed key-frame (k_schur_rows returns at once for its pieces, ha < 0); where a landmark is seen by
fewer key-frames than there are, the observation counts per key-frame are uneven and no multiple of 256."""
import collections
import functools

import numpy as np

from qsp_slam_amd import synth

PAIR_CAP = 4 << 20                    # entries of the key-frame pair lists (ba_solver.hip: PAIR_CAP)
KF_SQ_CAP = 1 << 24
ROWS_MIN_EDGES = 65536                # SCHUR_ROWS_MIN_EDGES
LDS_MAX = 160 * 1024                  # SCHUR_ROW_LDS_MAX
KSPLIT_SMALL, KSPLIT, KSPLIT_SMALL_BELOW = 512, 2048, 1 << 18
NB = 64
PAIRS, POINTS, ROWS, NONE = 0, 1, 2, -1

DM = float(np.float32(np.sqrt(5.991)))      # the Huber deltas of tests/test_gpu_ba.py
DS = float(np.float32(np.sqrt(7.815)))
DO = float(np.float32(np.sqrt(1e3)))


def pad(dim):
    return (dim + NB - 1) // NB * NB


def row_lds(dimp):
    """bytes of dynamic LDS of a k_schur_rows workgroup"""
    return 8 * (6 * dimp + 6)


def eliminated(n_free, n_obj, allowed=True):
    """objects eliminated in front of the dense solve? (key-frames in front of the objects in the hessian order, as in every scene here)"""
    return bool(allowed and n_obj > 0 and n_free > 0 and 8 * 6 * pad(6 * n_free) <= LDS_MAX)


def dense_dimp(n_free, n_obj, allowed=True):
    return pad(6 * (n_free + (0 if eliminated(n_free, n_obj, allowed) else n_obj)))


def default_is_pairs(n_kf, pairs):
    return pairs <= PAIR_CAP and n_kf * n_kf <= KF_SQ_CAP


def predict(n_edge, pairs, n_kf, n_free, n_obj, deterministic=None, elimination=True):
    """the form a trial takes.  deterministic: None = the mode qsp_ba_create chose, True / False = after set_deterministic (True
    beyond the cap is refused and leaves the mode as it was)"""
    dimp = dense_dimp(n_free, n_obj, elimination)
    if dimp == 0:
        return NONE
    det = default_is_pairs(n_kf, pairs) if deterministic is None else (bool(deterministic) and default_is_pairs(n_kf, pairs))
    if det and pairs > 0:
        return PAIRS
    return ROWS if (n_edge >= ROWS_MIN_EDGES and row_lds(dimp) <= LDS_MAX) else POINTS


def ksplit(n_edge):
    return KSPLIT_SMALL if n_edge < KSPLIT_SMALL_BELOW else KSPLIT


Counts = collections.namedtuple("Counts", "n_edge pairs n_kf n_free n_obj obs_per_kf")


def counts(sc):
    """what predict() needs, from the scene's arrays (every object of a scene here has edges)"""
    n_kf, n_pt = len(sc["kf_pose"]), len(sc["pt_xyz"])
    pt = np.concatenate([sc["mono_pt"], sc["st_pt"]])
    kf = np.concatenate([sc["mono_kf"], sc["st_kf"]])
    k = np.bincount(pt, minlength=n_pt).astype(np.int64)
    seen = np.bincount(kf, minlength=n_kf) + np.bincount(sc["oe_kf"], minlength=n_kf)
    n_free = int(((seen > 0) & (np.asarray(sc["kf_fixed"]) == 0)).sum())
    return Counts(len(pt), int((k * (k + 1) // 2).sum()), n_kf, n_free, len(np.unique(sc["oe_obj"])), np.bincount(kf, minlength=n_kf))


# ---- scenes: synth.make_ba_scene_large and four small edits of its arrays ------------------------------------------------------

def _drop_edges(sc, mask):
    sc = dict(sc)
    for k in ("mono_pt", "mono_kf", "mono_obs", "mono_info"):
        sc[k] = sc[k][~mask]
    return sc


def _fix(sc, n_fixed):
    sc = dict(sc)
    f = np.zeros(len(sc["kf_pose"]), np.uint8)
    f[:n_fixed] = 1
    sc["kf_fixed"] = f
    return sc


def _stereo(sc, frac, rng):
    """a fraction of the mono edges becomes stereo: u_right = u - bf / z at the true depth, one pixel of noise"""
    from qsp_slam_amd.synth import pose7_to_T
    sc = dict(sc)
    m = rng.random(len(sc["mono_pt"])) < frac
    T = np.array([pose7_to_T(p) for p in sc["gt_kf"]])
    kf, pt = sc["mono_kf"][m], sc["mono_pt"][m]
    z = np.einsum("ej,ej->e", T[kf, 2, :3], sc["gt_pt"][pt]) + T[kf, 2, 3]
    bf = sc["kf_K"][kf, 4]
    ur = sc["mono_obs"][m, 0] - bf / z + rng.normal(size=len(z))
    sc["st_pt"], sc["st_kf"] = pt.astype(np.int32), kf.astype(np.int32)
    sc["st_obs"] = np.concatenate([sc["mono_obs"][m], ur[:, None]], 1).astype(np.float32).astype(np.float64)
    sc["st_info"] = sc["mono_info"][m].copy()
    return _drop_edges(sc, m)


LOST_PT, LONE_PT = 11, 17             # rows_levels: a landmark whose every edge is a gross outlier / a landmark with a single edge


def _outliers(sc, frac, rng):
    """gross errors of 40..120 pixels in both image directions on a fraction of the edges and on every edge of LOST_PT"""
    sc = dict(sc)
    for pre in ("mono", "st"):
        obs = sc[pre + "_obs"].copy()
        bad = (rng.random(len(obs)) < frac) | (sc[pre + "_pt"] == LOST_PT)
        obs[bad, :2] += rng.uniform(40, 120, size=(int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2))
        sc[pre + "_obs"] = obs.astype(np.float32).astype(np.float64)
    return sc


def _single_edge(sc, pt):
    """landmark `pt` keeps its first mono edge only"""
    e = np.nonzero(sc["mono_pt"] == pt)[0]
    m = np.zeros(len(sc["mono_pt"]), bool)
    m[e[1:]] = True
    sc = _drop_edges(sc, m)
    s = sc["st_pt"] != pt
    for k in ("st_pt", "st_kf", "st_obs", "st_info"):
        sc[k] = sc[k][s]
    return sc


Spec = collections.namedtuple("Spec", "seed n_kf n_fixed n_pt obs n_obj stereo outliers drop_last form n_edge regime")

# name -> scene and the regime it is the smallest of.  `form` is the one set_deterministic(False) must give (for cap_*: the default
# mode as well); n_edge is asserted.  The seeds are ones for which the ORACLE ALONE (tests/test_oracle_ba_schur.py, no GPU in the
# loop) accepts every iteration of optimize(2) with the Huber kernels and of optimize(1) without at its first trial, and for which
# its dense and block-sparse solvers agree to 1e-12 in chi2 and states; rows_levels in addition leaves LOST_PT without an active
# edge at the stage boundary of local_joint_ba().  The first seed tried (23) met all of it on every scene.
TABLE = collections.OrderedDict([
    ("points_last",       Spec(23, 9, 1, 8192, 8, 2, 0.0, 0.0, True, POINTS, 65535, "last size of k_schur_points")),
    ("rows_first",        Spec(23, 9, 1, 8192, 8, 2, 0.0, 0.0, False, ROWS, 65536, "first size of k_schur_rows: 512-edge pieces, 15 per key-frame")),
    ("rows_mixed",        Spec(23, 9, 1, 8250, 8, 3, 0.3, 0.0, False, ROWS, 66000, "block rows, stereo edges, k_obj_prepare / k_obj_rows behind them or the objects in the dense system")),
    ("rows_levels",       Spec(23, 9, 1, 8250, 8, 3, 0.3, 0.1, False, ROWS, 65993, "local_joint_ba: block rows over level-1 edges, an inactive landmark, a single-edge landmark")),
    ("rows_lds_last",     Spec(23, 567, 2, 2400, 28, 3, 0.0, 0.0, False, ROWS, 67200, "dimp 3392: the largest row block that fits the LDS")),
    ("rows_lds_over",     Spec(23, 568, 2, 2400, 28, 3, 0.0, 0.0, False, POINTS, 67200, "dimp 3456: no row block fits, k_schur_points at a large edge count, objects in the dense system")),
    ("cap_points",        Spec(23, 300, 1, 94, 300, 2, 0.0, 0.0, False, POINTS, 28200, "above PAIR_CAP: the default mode is atomic, per landmark")),
    ("cap_rows",          Spec(23, 300, 1, 220, 300, 2, 0.0, 0.0, False, ROWS, 66000, "above PAIR_CAP: the default mode is atomic, block rows; 300 observations per landmark")),
    ("split_small_last",  Spec(23, 9, 1, 32768, 8, 2, 0.0, 0.0, True, ROWS, 262143, "last size of the 512-edge pieces")),
    ("split_large_first", Spec(23, 9, 1, 32768, 8, 2, 0.0, 0.0, False, ROWS, 262144, "first size of the 2048-edge pieces")),
])
NAMES = list(TABLE)
MID = ["points_last", "rows_first", "rows_mixed", "cap_points", "cap_rows"]     # optimize(2) robust + optimize(1) plain, against the oracle
LDS = ["rows_lds_last", "rows_lds_over"]                                        # the same runs, against the pair-list mode (see the GPU test)
SPLIT = ["split_small_last", "split_large_first"]                               # one iteration
ALSO_PAIRS = ["rows_first", "rows_mixed", "rows_levels"]                        # run in the pair-list mode as well
CAP = ["cap_points", "cap_rows"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """built once per session; nobody writes into it (both problem classes copy what they keep)"""
    s = TABLE[name]
    rng = np.random.default_rng(1000 + s.seed)
    sc = synth.make_ba_scene_large(s.seed, s.n_kf, s.n_pt, obs_per_pt=s.obs, n_obj=s.n_obj)
    sc = _fix(sc, s.n_fixed)
    if s.stereo:
        sc = _stereo(sc, s.stereo, rng)
    if s.outliers:
        sc = _single_edge(_outliers(sc, s.outliers, rng), LONE_PT)
    if s.drop_last:
        m = np.zeros(len(sc["mono_pt"]), bool)
        m[-1] = True
        sc = _drop_edges(sc, m)
    return sc


def rel(a, b, rtol, atol):
    """the effective relative error of np.allclose(a, b, rtol, atol): max |a - b| / (|b| + atol / rtol)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + atol / rtol)).max()) if a.size else 0.0


def moving(chi2):
    """iterations whose chi2 still moves by more than 1e-3 of itself: where lambda is compared
    (test_vertices_without_edges_and_single_observation_landmarks in tests/test_gpu_ba.py explains why)"""
    c = np.asarray(chi2, np.float64)
    return np.concatenate([[True], (c[:-1] - c[1:]) > 1e-3 * c[:-1]])[: len(c)]
