"""Cases of tests/test_gpu_ray_edges.py: the ray-sample list kernels of the render term (csrc/sdf_kernels.hpp: k_sample, k_scan,
k_stage_list and the plan tails) beyond one pass of rays and off 50 depth samples.  k_sample walks a hypothesis's rays 1024 at a
time, k_scan 512 (clearing and refilling its LDS row table from the second pass on), k_stage_list 256, each carrying list offsets
from pass to pass; depth indices are packed as (ray << 6) | k, the sample masks are 64-bit, the staged forward splits at D // 2.

Every case: the fitted decoder tests/golden/decoder_8x512.npz, synth.make_object_views(seed, 1, 64, n_fg, n_bg), code zero,
so.JointConfig(n_depth=D), one iteration of the float32 oracle (so.gn_iteration) with the float64 one beside it.

Membership in the unit ball, in the band |s| < cut_off and the keep rule de_do > 1e-2 are discrete decisions, and with tens of
thousands of samples the float32 oracle itself has samples within 1e-6 of a threshold (one seed had a norm of exactly 1.0): a GPU
evaluation that contracts one multiply-add differently would change n_valid or K for no kernel fault.  So the seed of every case
was chosen with the oracle alone, on the CPU, until `conditions` holds (tests/test_ray_edge_cases.py asserts it):
  1. every | |p| - 1 | >= 4e-6 (32 float32 ulps at 1.0: both sides evaluate the same float32 expressions);
  2. every | |s| - cut_off | of a valid sample >= 1e-5 (five times the decode bar of tests/test_gpu_sdf.py, 2e-6);
  3. every de_do of an in-band sample at least 1e-3 relative away from 1e-2;
  4. the float32 and the float64 oracle agree on n_valid, K and the row order;
  5. in every group of fewer than 50 render rows (groups: ray // 512; for the depth cases k < D // 2 and k >= D // 2) the
     Jacobian rows of the two oracles differ by at most half the row bar, for every row: no ReLU knife-edge row where the GPU test
     can excuse none;
  6. coverage: a kept row from a ray of every 512-ray pass (from the single ray of the last pass at 513 and 1025 rays), a ray
     with no valid sample, K >= 2 for D >= 4, a valid sample at k = 62 for D = 64.

CPU only: numpy, the oracle and the synthetic-scene generator."""
import functools
import os

import numpy as np

from oracle import sdf_oracle as so
from qsp_slam_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M_PTS = 64
SCAN_RAYS = 512                 # rays per pass of k_scan; k_sample takes 1024, k_stage_list 256
ROW_TOL, ROW_MAX_BAD = 2e-5, 0.02    # the render-row bars of tests/test_gpu_sdf.py::test_jacobian_rows_of_fused_kernel_vs_reference
SMALL_GROUP = 50                # a group of fewer rows allows no row out
RES_TOL = 1e-4                  # column 71 (the robust residual), of its largest value, every row
BALL_MARGIN, BAND_MARGIN, KEEP_MARGIN = 4e-6, 1e-5, 1e-3

# name: (n_fg, n_bg, D, seed)
CASES = {
    # A. ray passes at D = 50: all-foreground lists (only rays that hit the surface produce kept rows; a background ray in the last
    # pass would leave that pass's row emission unobserved); the last one is four k_scan, two k_sample, seven k_stage_list passes
    "r511": (511, 0, 50, 65),
    "r512": (512, 0, 50, 71),
    "r513": (513, 0, 50, 8566),
    "r1024": (1024, 0, 50, 192),
    "r1025": (1025, 0, 50, 93),
    "r1100+437": (1100, 437, 50, 28),
    # B. depth counts at 200 + 100 rays: D = 3 (only the centre plane can be valid), 4 and 5 (the first staged counts, k_mid = 2
    # both times), odd counts, 63 / 64 (bit 62 of the masks -- samples 0 and D - 1 lie ON the unit sphere and `< 1` is strict, so
    # k = 63 cannot be valid -- and the full row of the LDS table)
    "d3": (200, 100, 3, 1),
    "d4": (200, 100, 4, 2),
    "d5": (200, 100, 5, 1),
    "d7": (200, 100, 7, 1),
    "d49": (200, 100, 49, 3),
    "d63": (200, 100, 63, 1),
    "d64": (200, 100, 64, 1),
}
RAY_CASES = tuple(n for n in CASES if n.startswith("r"))
DEPTH_CASES = tuple(n for n in CASES if n.startswith("d"))
STAGED = ("r513", "r1100+437", "d3", "d4", "d5", "d63", "d64")      # screened / depth-staged against unscreened, bit for bit
# C. exits: render_none (fewer than 10 valid samples: at D = 2 both samples of every ray lie on the unit sphere), render_nan
# (n_valid >= 10 but no kept row, K = 0: reference optimizer.py:193-194), no rays at all
NONE_CASE = (200, 100, 2, 1)
NAN_CASE = (100, 50, 4, 1005, 200)        # (n_fg, n_bg, D, seed, n_pts): n_valid = 225, K = 0
RAGGED = (0, 40, 513, 1025)               # rays of the objects of the one ragged batch (all foreground, 64 points each)
RAGGED_SEED = 1


@functools.lru_cache(maxsize=None)
def oracle_decoder():
    return so.load_decoder_npz(os.path.join(GOLDEN, "decoder_8x512.npz"))


def make_object(seed, n_fg, n_bg, n_pts=M_PTS):
    o = synth.make_object_views(seed, 1, n_pts, n_fg=n_fg, n_bg=n_bg)[0]
    assert o["rays"].shape == (n_fg + n_bg, 3) and o["depth"].shape == (n_fg,)
    return o


def _iteration(fn, *args):
    """fn(*args) (so.gn_iteration / so.gn_iteration_f64) and what it handed to and got from so.render_term: (it, rt, call) with
    call = dict(depth_obs, T_oc, depths) -- the oracle's own intermediate values, not a second evaluation"""
    seen = {}
    orig = so.render_term

    def tap(dec, rays, depth_obs, T_oc, depths, code, th=0.01):
        seen["call"] = dict(dec=dec, rays=rays, depth_obs=depth_obs, T_oc=T_oc, depths=depths, code=code, th=th)
        seen["rt"] = orig(dec, rays, depth_obs, T_oc, depths, code, th=th)
        return seen["rt"]

    so.render_term = tap
    try:
        it = fn(*args)
    finally:
        so.render_term = orig
    return it, seen.get("rt"), seen.get("call")


def build(n_fg, n_bg, D, seed, n_pts=M_PTS):
    """dict(obj, cfg, D, n_fg, T0 (1,4,4), T_oc, dobs, it / rt / call: the float32 iteration, it64 / rt64: the float64 one)"""
    o = make_object(seed, n_fg, n_bg, n_pts)
    cfg = so.JointConfig(n_depth=D)
    T_oc = np.linalg.inv(o["t_cam_obj"].astype(np.float64)).astype(np.float32)
    dobs = np.concatenate([o["depth"], np.zeros(n_bg, np.float32)])
    args = (oracle_decoder(), cfg, T_oc, np.zeros(64, np.float32), o["pts"], o["rays"], dobs, n_fg)
    it, rt, call = _iteration(so.gn_iteration, *args)
    it64, rt64, _ = _iteration(so.gn_iteration_f64, *args)
    return dict(obj=o, cfg=cfg, D=D, n_fg=n_fg, n_rays=n_fg + n_bg, T0=o["t_cam_obj"][None], T_oc=T_oc, dobs=dobs, it=it, rt=rt, call=call,
                it64=it64, rt64=rt64)


@functools.lru_cache(maxsize=None)
def build_case(name):
    """the case's scene and oracle iterations, computed once per process and shared (read-only) by every test that needs them"""
    n_fg, n_bg, D, seed = CASES[name]
    c = build(n_fg, n_bg, D, seed)
    c["name"] = name
    return c


def row_groups(case):
    """group index per kept render row: the k_scan pass of its ray, or for a depth case the stage of its depth index"""
    rt = case["rt"]
    if case["name"].startswith("d"):
        return (rt["k"] >= case["D"] // 2).astype(np.int64), 2
    return rt["ray"] // SCAN_RAYS, (case["n_rays"] + SCAN_RAYS - 1) // SCAN_RAYS


def row_errors(a, b):
    """per row: the largest |a - b| of the row over the largest |b| of the matrix (tests/test_oracle_sdf.py:rows_close's measure)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).reshape(a.shape[0], -1).max(1) / max(np.abs(b).max(), 1e-30)


def jacobian_row_errors(Jp, Jc, it):
    """per render row, the larger of row_errors on the pose block and on the code block (the fixture test holds each to its bar)"""
    return np.maximum(row_errors(Jp, it["Jp_render"]), row_errors(Jc, it["Jc_render"]))


def grouped_rows_ok(err, groups, n_groups):
    """rows_close(tol=ROW_TOL, max_bad=ROW_MAX_BAD) per group of rows, a group of fewer than SMALL_GROUP rows with no row out -- a
    wrong last pass of two rows must not hide inside 2 % of 500; returns (ok, worst error, worst error of a small group)"""
    ok, small = True, 0.0
    for g in range(n_groups):
        e = err[groups == g]
        if e.size == 0:
            continue
        if e.size < SMALL_GROUP:
            small = max(small, float(e.max()))
            ok = ok and bool((e <= ROW_TOL).all())
        else:
            ok = ok and bool((e > ROW_TOL).mean() <= ROW_MAX_BAD)
    return ok, float(err.max()) if err.size else 0.0, small


def in_band_de_do(case):
    """de_do of EVERY in-band sample of the float32 iteration (so.render_term keeps those above 1e-2 only): its lines 246-262 on the
    sample values it returned"""
    rt, c = case["rt"], case["call"]
    F = np.float32
    R, D = c["rays"].shape[0], c["depths"].shape[0]
    s, vr, vk, th = rt["sdf_valid"], rt["valid_ray"], rt["valid_k"], F(c["th"])
    occ = np.zeros((R, D), F)
    occ[vr, vk] = F(0.5) - np.clip(s, -th, th) / (F(2) * th)
    wg = (s > -th) & (s < th)
    gr, gk = vr[wg], vk[wg]
    acc = np.cumprod(F(1) - occ[gr, :], axis=-1, dtype=F)
    acc_m = np.where(np.arange(D)[None, :] < gk[:, None], F(0), acc)
    return acc_m.sum(-1, dtype=F) / (F(1) - occ[gr, gk]), gr, gk


def decision_margins(case):
    """how far the float32 iteration's discrete decisions are from their thresholds: min | |p| - 1 | over every ray sample, min
    | |s| - cut_off | over the valid ones, min | de_do / 1e-2 - 1 | over the in-band ones (1.0 where there is none)"""
    rt, c = case["rt"], case["call"]
    p = so.transform_points(c["T_oc"], c["rays"][:, None, :] * c["depths"][:, None])
    norm = np.sqrt((p * p).sum(-1, dtype=np.float32))
    fig = dict(ball=float(np.abs(norm.astype(np.float64) - 1.0).min()), band=1.0, keep=1.0)
    if rt is not None:
        de_do, gr, gk = in_band_de_do(case)
        kept = de_do > 1e-2
        assert np.array_equal(gr[kept], rt["ray"]) and np.array_equal(gk[kept], rt["k"])     # (the restatement is the oracle's)
        fig["band"] = float(np.abs(np.abs(rt["sdf_valid"].astype(np.float64)) - c["th"]).min())
        if de_do.size:
            fig["keep"] = float(np.abs(de_do.astype(np.float64) / 1e-2 - 1.0).min())
    return fig


def margins_hold(fig):
    return fig["ball"] >= BALL_MARGIN and fig["band"] >= BAND_MARGIN and fig["keep"] >= KEEP_MARGIN


def conditions(case):
    """the measured figures of conditions 1..6 (module docstring) for a case with a render term"""
    it, it64, rt, rt64 = case["it"], case["it64"], case["rt"], case["rt64"]
    n_rays = case["n_rays"]
    fig = dict(decision_margins(case), n_valid=it["n_valid"], K=it["K"])
    fig["same_lists"] = bool(it64["fail"] is None and it64["n_valid"] == it["n_valid"] and it64["K"] == it["K"] and
                             np.array_equal(rt64["ray"], rt["ray"]) and np.array_equal(rt64["k"], rt["k"]) and
                             np.array_equal(rt64["valid_ray"], rt["valid_ray"]) and np.array_equal(rt64["valid_k"], rt["valid_k"]))
    groups, n_groups = row_groups(case)
    fig["rows_per_group"] = [int((groups == g).sum()) for g in range(n_groups)]
    if fig["same_lists"]:
        err = jacobian_row_errors(it["Jp_render"], it["Jc_render"], it64)
        fig["small_group_rows"] = max([float(err[groups == g].max()) for g in range(n_groups) if 0 < (groups == g).sum() < SMALL_GROUP],
                                      default=0.0)
        fig["rows"] = float(err.max())
    fig["rays_without_sample"] = int(n_rays - np.unique(rt["valid_ray"]).size)
    fig["last_ray_kept"] = bool((rt["ray"] == n_rays - 1).any())
    fig["top_k"] = int(rt["valid_k"].max())
    return fig


def conditions_hold(case, fig):
    name = case["name"]
    ok = (margins_hold(fig) and fig["same_lists"] and
          fig.get("small_group_rows", 1.0) <= 0.5 * ROW_TOL and fig["rays_without_sample"] >= 1)
    if name.startswith("r"):
        ok = ok and min(fig["rows_per_group"]) >= 1
        if case["n_rays"] % SCAN_RAYS == 1:
            ok = ok and fig["last_ray_kept"] and fig["rows_per_group"][-1] >= 1
    else:
        if case["D"] >= 4:
            ok = ok and fig["K"] >= 2
        if case["D"] == 64:
            ok = ok and fig["top_k"] == 62
    return bool(ok)


def opaque_before_mid(case):
    """rays of the float32 iteration with an opaque sample (sdf <= -cut_off: occupancy exactly 1) in front of k_mid = D // 2 that
    also have a valid sample at or behind it: the samples a depth-staged forward does not evaluate"""
    rt, th, k_mid = case["rt"], np.float32(case["call"]["th"]), case["D"] // 2
    closed = np.unique(rt["valid_ray"][(rt["valid_k"] < k_mid) & (rt["sdf_valid"] <= -th)])
    return int((np.isin(rt["valid_ray"], closed) & (rt["valid_k"] >= k_mid)).sum())


def no_ray_object():
    """an object whose `rays` have shape (0, 3)"""
    o = dict(make_object(RAGGED_SEED, 40, 0))
    o["rays"], o["depth"] = np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    return o


def ragged_objects():
    objs = [no_ray_object()] + [make_object(RAGGED_SEED + i, n, 0) for i, n in enumerate(RAGGED) if n > 0]
    assert tuple(o["rays"].shape[0] for o in objs) == RAGGED
    return objs
