"""The cases of the pose-only refinement tests (Optimizer.estimate_pose_cam_obj, reconstruct/optimizer.py:47-93), computed once and
shared by tests/test_oracle_pose_only.py (CPU) and tests/test_gpu_pose_only.py (GPU).

A case is one object of synth.make_object_views with its perturbed start pose and a non-zero code of norm about 0.05 x sqrt(L); no
rays.  The oracle (oracle/sdf_oracle.py:estimate_pose_cam_obj) runs every case for 8 iterations with its trace, so that the runs of
5 and 6 iterations are prefixes of it: record e holds the state before iteration e, H, b, dx, the residuals, the state after it and
the same iteration evaluated in float64 from the same float32 state (the yardstick); record 4 also holds the kept mask of the
inlier filter.

The tests compare STEPS, not poses: step(T_before, T_after) = T_after inv(T_before) on the object-from-camera matrices (scale baked
in as the library and the reference bake it, optimizer.py:57-58, and taken out as in :88), at
step_err = |step_a - step_b|_max / max(|step_b - I|_max, 1e-6)."""
import functools
import os

import numpy as np

from oracle import sdf_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_ITER = 8                       # every oracle trace; the filter acts behind iteration index 4
KNIFE_EDGE = 1e-3                # no residual of iteration 4 closer than this to the filter's 0.05
BAR_FLOOR = 1e-4                 # the project's bar on H, b and poses
BAR_FACTOR = 4.0                 # the margin the other oracle tests give over the oracle's own rounding
STEP_FLOOR = 1e-6

SINGLE_SIZES = (1, 31, 33, 63, 64, 65, 129, 300)
NARROW_SIZES = (33, 65)
PIPE_SIZES = (1, 33, 64, 65, 129)                                    # the single cases that also run on the split pipes
FORMS = (("f32", 64), ("bf16x3", 64), ("fp16x2", 64), ("fp16x2", 32))
NARROW_FORMS = (("fp16x2", 64), ("fp16x2", 32))
RAGGED = ("m65", "m1", "filter_m300", "m64", "emptied_m33", "m129")     # one qsp_estimate_pose call


def _spec():
    """name -> dict(m, seed, decoder, outliers): the seeds are chosen so that every case clears the knife-edge rule"""
    s = {}
    for m in SINGLE_SIZES:
        s["m%d" % m] = dict(m=m, seed=9100 + m, decoder="big", outliers=None)
    for m in NARROW_SIZES:
        s["narrow_m%d" % m] = dict(m=m, seed=9500 + m, decoder="small", outliers=None)
    s["filter_m65"] = dict(m=65, seed=9765, decoder="big", outliers="every7th")
    s["filter_m300"] = dict(m=300, seed=77, decoder="big", outliers="every7th")      # the object of tests/test_gpu_sdf.py's filter test
    s["emptied_m33"] = dict(m=33, seed=9833, decoder="big", outliers="all")
    return s


SPEC = _spec()
SINGLE = tuple("m%d" % m for m in SINGLE_SIZES) + tuple("narrow_m%d" % m for m in NARROW_SIZES)
FILTER = ("filter_m65", "filter_m300")
EMPTIED = "emptied_m33"
ALL = tuple(SPEC)


@functools.lru_cache(maxsize=None)
def oracle_decoder(which):
    return so.load_decoder_npz(os.path.join(GOLDEN, "decoder_8x512.npz" if which == "big" else "decoder_4x256_c32.npz"))


def se3_and_scale(t_cam_obj):
    """a Sim3 object->camera matrix as the (SE3 float32, scale) pair estimate_pose_cam_obj takes"""
    T = np.asarray(t_cam_obj, np.float64)
    s = np.linalg.det(T[:3, :3]) ** (1.0 / 3.0)
    T = T.copy()
    T[:3, :3] /= s
    return T.astype(np.float32), float(np.float32(s))


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one estimate_pose_cam_obj call (left unchanged by everyone)"""
    from qsp_slam_amd import synth
    sp = SPEC[name]
    L = 64 if sp["decoder"] == "big" else 32
    o = synth.make_object_views(sp["seed"], 1, sp["m"], n_fg=8, n_bg=4)[0]
    t_co_se3, scale = se3_and_scale(o["t_cam_obj"])
    pts = o["pts"].copy()
    if sp["outliers"] == "every7th":
        pts[::7] += np.float32(0.25)                  # gross outliers: SDF residual > 0.05
    elif sp["outliers"] == "all":
        # a shell at three times the object's size around its centre: no rigid motion brings any of it near the surface
        c = o["gt_t_cam_obj"][:3, 3].astype(np.float32)
        pts = (c + np.float32(3.0) * (pts - c)).astype(np.float32)
    code = (0.05 * np.random.default_rng(sp["seed"]).standard_normal(L)).astype(np.float32)
    for a in (t_co_se3, pts, code):
        a.setflags(write=False)
    return dict(name=name, L=L, decoder=sp["decoder"], t_co_se3=t_co_se3, scale=scale, pts=pts, code=code)


@functools.lru_cache(maxsize=None)
def run(name):
    """the oracle's 8 iterations of a case: dict(case, trace, kept, n_done).  The emptied object's trace ends with iteration 4 (the
    reference then divides by zero): n_done = 5."""
    c = case(name)
    cfg = so.JointConfig(n_iter_pose=N_ITER, code_len=c["L"])
    n_it = 5 if name == EMPTIED else N_ITER
    cfg.n_iter_pose = n_it
    trace = []
    so.estimate_pose_cam_obj(oracle_decoder(c["decoder"]), cfg, c["t_co_se3"], c["scale"], c["pts"], c["code"], trace=trace,
                             trace_f64=True)
    return dict(case=c, trace=trace, kept=trace[4]["kept"], n_done=n_it)


def oracle_pose(name, n_iter):
    """what the oracle returns after n_iter iterations: the (4,4) float32 SE3 t_cam_obj (optimizer.py:84-90)"""
    r = run(name)
    T_oc = r["trace"][n_iter - 1]["T_oc_new"]
    T_co = np.linalg.inv(T_oc).astype(np.float32)
    T_co[:3, :3] /= np.float32(r["case"]["scale"])
    return T_co


# ---- steps ------------------------------------------------------------------------------------------------------------------

def T_oc_of(t_co_se3, scale):
    """the object-from-camera matrix of an (SE3, scale) pair, float64: the scale is baked in float32 as the library and the oracle
    bake it, the inverse is exact"""
    T = np.array(t_co_se3, np.float32).reshape(4, 4)
    T[:3, :3] *= np.float32(scale)
    return np.linalg.inv(T.astype(np.float64))


def start_of(T_oc, scale):
    """the float32 SE3 t_cam_obj that starts a call at the object-from-camera state T_oc"""
    T = np.linalg.inv(np.asarray(T_oc, np.float64))
    T[:3, :3] /= float(np.float32(scale))
    return T.astype(np.float32)


def step(T_before, T_after):
    return np.asarray(T_after, np.float64) @ np.linalg.inv(np.asarray(T_before, np.float64))


def step_err(s, s_ref):
    return float(np.abs(s - s_ref).max() / max(np.abs(s_ref - np.eye(4)).max(), STEP_FLOOR))


def oracle_step(name, e, flavour="f32"):
    it = run(name)["trace"][e]
    if flavour == "f64":
        it = it["f64"]
    return step(it["T_oc"], it["T_oc_new"])


def yardstick(name, e):
    """the float32 oracle's own distance from its float64 flavour on the step of iteration e"""
    return step_err(oracle_step(name, e), oracle_step(name, e, "f64"))


def bar(name, e):
    return max(BAR_FACTOR * yardstick(name, e), BAR_FLOOR)


def points_of(name, e):
    """the points iteration e of the oracle runs on: all of them up to iteration 4, the kept ones behind it"""
    r = run(name)
    return r["case"]["pts"] if e <= 4 else r["case"]["pts"][r["kept"]]


def defect_steps(name, e):
    """the oracle's step of iteration e recomputed with a tile kernel's possible defects: the last point left out or counted twice
    (the divisor stays the count of active points, which the solve kernel takes from the mask), and -- behind the filter -- the
    divisor left at the uploaded count"""
    r = run(name)
    c, it = r["case"], r["trace"][e]
    dec = oracle_decoder(c["decoder"])
    pts = points_of(name, e)
    n = pts.shape[0]
    out = dict(last_point_left_out=so.pose_only_iteration(dec, it["T_oc"], c["code"], pts[:-1], divisor=n),
               last_point_twice=so.pose_only_iteration(dec, it["T_oc"], c["code"], np.concatenate([pts, pts[-1:]]), divisor=n))
    if e > 4 and n != c["pts"].shape[0]:
        out["divisor_at_uploaded_count"] = so.pose_only_iteration(dec, it["T_oc"], c["code"], pts, divisor=c["pts"].shape[0])
    return {k: step(v["T_oc"], v["T_oc_new"]) for k, v in out.items()}
