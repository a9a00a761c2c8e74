"""Call sequences on ONE long-lived bundle-adjustment problem, shared by tests/test_oracle_ba_sequences.py (the C oracle driven
through them on the CPU: does each sequence reach what it is meant to reach?) and tests/test_gpu_ba_reuse.py (the GPU problem
driven through the same steps and compared step by step).

A sequence is a list of steps.  `run()` drives either kind of problem through it: qsp_slam_amd.ba.BaProblem and
oracle.ba_oracle.BaProblem answer the same calls for everything that touches levels or estimates.  The SOLVER_OPTIONS steps
(sharding, deterministic mode, object elimination, the form of the factorisation) exist on the GPU problem only; by the contract
of include/qsp_hip.h they change how the next solve is computed and never levels or estimates, so the oracle skips them -- which
is exactly why the unsharded oracle sequence is the reference of a sharded GPU sequence."""
import functools

import numpy as np

from oracle import ba_oracle as bo
from qsp_slam_amd import synth

DM = float(np.float32(np.sqrt(5.991)))
DS = float(np.float32(np.sqrt(7.815)))
DO = float(np.float32(np.sqrt(1e3)))

C2 = dict(seed=32, n_kf=20, n_pt=2000, n_obj=8, stereo_frac=0.2)                  # BASELINE config 2 shape
SHARDED = dict(seed=61, n_kf=10, n_pt=400, n_obj=3, stereo_frac=0.3, outlier_frac=0.06)


def device_boundary_scene():
    """an ordinary scene with outliers: no pose vertex loses its last edge at the stage boundary of a local BA -> device path"""
    return synth.make_ba_scene(**dict(C2, outlier_frac=0.08))


def host_boundary_scene():
    """one object's camera-object measurements are mutually inconsistent (each off by metres in its own direction): after the
    first stage every one of its edges is an outlier, the object vertex leaves the index, the reduced system shrinks -> host path"""
    sc = synth.make_ba_scene(**dict(C2, outlier_frac=0.05))
    rng = np.random.default_rng(8)
    meas = sc["oe_meas"].copy()
    mine = np.nonzero(sc["oe_obj"] == 0)[0]
    meas[mine, :3] += rng.normal(scale=4.0, size=(len(mine), 3))
    sc["oe_meas"] = meas
    return sc


def sharded_scene():
    return synth.make_ba_scene(**SHARDED)


SCENES = dict(device=device_boundary_scene, host=host_boundary_scene, sharded=sharded_scene)


@functools.lru_cache(maxsize=None)
def scene(name):
    """built once per session; nobody writes into it (both problem classes copy what they keep)"""
    return SCENES[name]()


def custom_levels(sc):
    """every edge of landmark 0 at level 1: the landmark leaves the index (g2o's active-vertex rule)"""
    return (sc["mono_pt"] == 0).astype(np.uint8), (sc["st_pt"] == 0).astype(np.uint8), None


# ---- steps ---------------------------------------------------------------------------------------------------------------------
LJ = ("local_joint",)
LJ_STOPPED = ("local_joint_stopped",)           # the stop flag is up at the call: it returns with nothing touched
STATE0 = ("set_state_initial",)
LEVELS_NONE = ("set_levels", "none")
LEVELS_CUSTOM = ("set_levels", "custom")
INDEX = ("index",)
EDGES = ("edges",)


def OPT(n, dm=DM, ds=DS, do=DO):
    return ("optimize", n, dm, ds, do)


SOLVER_OPTIONS = ("set_shard", "set_deterministic", "set_object_elimination", "set_cholesky_chain")
SHARD_OWN, SHARD_OTHER, SHARD_OFF = ("set_shard", "own"), ("set_shard", "other"), ("set_shard", "off")
DET_ON, DET_OFF = ("set_deterministic", True), ("set_deterministic", False)
ELIM_ON, ELIM_OFF = ("set_object_elimination", True), ("set_object_elimination", False)
CHAIN_OFF = ("set_cholesky_chain", False)

# name -> (scene, steps).  A-I: one rank.  S1-S4: two ranks, each with a problem of its own ("own" = set_shard(rank, 2),
# "other" = set_shard(1 - rank, 2), "off" = set_shard(0, 1)).
SEQUENCES = {
    "A": ("device", [LJ, OPT(3), INDEX]),
    "B": ("device", [LJ, EDGES, INDEX]),
    "C": ("device", [LJ, LEVELS_CUSTOM, OPT(2, 0.0, 0.0, 0.0), INDEX]),
    "D": ("host", [LJ, STATE0, LJ, INDEX]),
    "E": ("device", [LJ, ELIM_OFF, STATE0, LJ, ELIM_ON, STATE0, LJ, INDEX]),
    "F": ("sharded", [DET_ON, LEVELS_CUSTOM, OPT(3), LEVELS_NONE, STATE0, OPT(3)]),
    "G": ("device", [DET_ON, STATE0, LJ, DET_OFF, STATE0, LJ, DET_ON, STATE0, LJ]),
    "H": ("sharded", [LJ_STOPPED, LJ]),
    "I": ("device", [LJ, CHAIN_OFF, STATE0, LJ]),
    "S1": ("sharded", [LEVELS_NONE, SHARD_OWN, OPT(4)]),
    "S2": ("sharded", [LJ, SHARD_OWN, OPT(3), INDEX]),
    "S3": ("sharded", [SHARD_OWN, LJ, INDEX, SHARD_OTHER, OPT(3), INDEX]),
    "S4": ("sharded", [SHARD_OWN, LJ, SHARD_OFF, DET_ON, STATE0, LJ]),
}


def run(p, sc, steps, solver_option=None):
    """Drive problem `p` (created from scene `sc`) through `steps`; one record per step (None for a step that returns nothing).
    solver_option(p, step) applies a SOLVER_OPTIONS step; None skips those steps (the oracle)."""
    out = []
    for st in steps:
        op, rec = st[0], None
        if op in SOLVER_OPTIONS:
            if solver_option is not None:
                solver_option(p, st)
        elif op == "local_joint":
            t1, t2 = p.local_joint_ba()
            rec = dict(t1=t1, t2=t2, state=p.state())
        elif op == "local_joint_stopped":
            p.local_joint_ba(stop=np.ones(1, np.uint8))
            rec = dict(state=p.state())
        elif op == "optimize":
            t = p.optimize(*st[1:])
            rec = dict(t=t, state=p.state())
        elif op == "set_state_initial":
            p.set_state(sc["kf_pose"], sc["pt_xyz"], sc["obj_pose"])
        elif op == "set_levels":
            p.set_levels(*((None, None, None) if st[1] == "none" else custom_levels(sc)))
        elif op == "index":
            rec = dict(index=p.index())
        elif op == "edges":
            rec = dict(edges=p.edges())
        else:
            raise ValueError("unknown step %r" % (st,))
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the C oracle driven through SEQUENCES[name], once per session; (records, levels after every step).  Read-only."""
    sname, steps = SEQUENCES[name]
    sc = scene(sname)
    ref = bo.BaProblem(sc)
    recs, levels = [], []
    for st in steps:
        recs += run(ref, sc, [st])
        levels.append(ref.levels())
    return recs, levels


def takes_device_boundary(rec):
    """what the library's device-side stage boundary needs, read off a local_joint record of the oracle: the first stage ran its
    five iterations, its last trial was accepted, and no key-frame or object vertex changed its place in the index"""
    t1, t2 = rec["t1"], rec["t2"]
    return (len(t1["chi2"]) == 5 and int(t1["accepted"][-1]) == 1 and np.array_equal(t1["kf_hidx"], t2["kf_hidx"])
            and np.array_equal(t1["obj_hidx"], t2["obj_hidx"]))
