"""One long-lived qsp_ba_problem driven through the call sequences of tests/ba_sequences.py and compared step by step: levels,
sharding and options must survive any of these orders (the contract at qsp_ba_set_shard / qsp_ba_set_levels in include/qsp_hip.h;
DESIGN.md, "lifetime of a BA problem").  Behind the C-ABI sit four pieces of lazily synchronised state -- the deferred level reset
of set_levels(NULL..), the host copies that lag a device-side stage boundary, the cached all-active index, and what the device
holds of the index tables -- and a fresh problem with one call, which is what tests/test_gpu_ba.py mostly uses, exercises none of
them.

Reference: the C oracle driven through the SAME sequence (tests/test_oracle_ba_sequences.py shows on the CPU that every sequence
reaches what it is meant to reach); for the sharded steps the unsharded oracle sequence -- set_shard must not change the
mathematics.  Bars are those of tests/test_gpu_ba.py through its close(): index tables, trials, accept flags and results exact;
chi2 1e-8; lambda 1e-8 (1e-7 sharded); estimates rtol 1e-7 / atol 1e-9; per-edge chi2 rtol 1e-7 / atol 1e-9.  Where a step
repeats arithmetic that already ran (same problem or a fresh one, atomic-free Schur complement) the bar is np.array_equal."""
import threading

import numpy as np
import pytest

from tests import ba_sequences as seq
from tests.test_gpu_ba import close

pytestmark = pytest.mark.gpu


def _option(rank=0, comm=None):
    """applies the SOLVER_OPTIONS steps to a GPU problem of rank `rank` (two ranks: threads on the one GPU, ThreadAllreduce)"""
    def apply(p, st):
        op, arg = st
        if op == "set_shard":
            if arg == "off":
                p.set_shard(0, 1, None)
            else:
                r = rank if arg == "own" else 1 - rank
                p.set_shard(r, 2, comm.hook(rank))      # (the hook's slot is the THREAD's; the shard it computes is r's)
        elif op == "set_deterministic":
            p.set_deterministic(arg)
        elif op == "set_object_elimination":
            p.set_object_elimination(arg)
        elif op == "set_cholesky_chain":
            p.set_cholesky_chain(arg)
    return apply


def _same_trace(g, r, lam_rtol=1e-8):
    assert list(g["trials"]) == list(r["trials"]) and list(g["accepted"]) == list(r["accepted"])
    assert g["result"] == r["result"] and g["iterations"] == r["iterations"]
    assert close(g["chi2"], r["chi2"], rtol=1e-8)
    assert close(g["lam"], r["lam"], rtol=lam_rtol)
    if "pt_hidx" in g:
        _same_index((g["kf_hidx"], g["obj_hidx"], g["pt_hidx"]), (r["kf_hidx"], r["obj_hidx"], r["pt_hidx"]))
    # the sizes the library reports for the solve are those of the oracle's index tables
    assert g["n_pose_blocks"] == int((r["kf_hidx"] >= 0).sum() + (r["obj_hidx"] >= 0).sum())
    assert g["n_landmarks"] == int((r["pt_hidx"] >= 0).sum())


def _same_index(g, r):
    for a, b in zip(g, r):
        assert np.array_equal(a, b)


def _same_state(g, r):
    for a, b in zip(g, r):
        assert close(a, b, rtol=1e-7, atol=1e-9)


def _against_oracle(name, got):
    """every record of a GPU run of SEQUENCES[name] against the oracle's record of the same step"""
    want, _ = seq.oracle_run(name)
    steps = seq.SEQUENCES[name][1]
    assert len(got) == len(want) == len(steps)
    lam_rtol = 1e-8
    for st, g, r in zip(steps, got, want):
        assert (g is None) == (r is None), st
        if st[0] == "set_shard":        # (sums re-associated across ranks: lambda to 1e-7 while the problem is sharded)
            lam_rtol = 1e-8 if st[1] == "off" else 1e-7
        if st[0] == "local_joint":
            _same_trace(g["t1"], r["t1"], lam_rtol)
            _same_trace(g["t2"], r["t2"], lam_rtol)
            _same_state(g["state"], r["state"])
        elif st[0] == "optimize":
            _same_trace(g["t"], r["t"], lam_rtol)
            _same_state(g["state"], r["state"])
        elif st[0] == "index":
            _same_index(g["index"], r["index"])
        elif st[0] == "edges":
            assert close(g["edges"]["mono_chi2"], r["edges"]["mono_chi2"], rtol=1e-7, atol=1e-9)
            assert close(g["edges"]["st_chi2"], r["edges"]["st_chi2"], rtol=1e-7, atol=1e-9)
            assert close(g["edges"]["oe_chi2"], r["edges"]["oe_chi2"], rtol=1e-7, atol=1e-9)
            assert np.array_equal(g["edges"]["mono_pos"], r["edges"]["mono_pos"])
            assert np.array_equal(g["edges"]["st_pos"], r["edges"]["st_pos"])


def _bits(rec):
    """everything a local_joint / optimize record holds, for np.array_equal"""
    tr = [rec[k] for k in ("t1", "t2", "t") if k in rec]
    out = list(rec["state"])
    for t in tr:
        out += [np.asarray(t["chi2"]), np.asarray(t["lam"]), np.asarray(t["trials"]), np.asarray(t["accepted"])]
    return out


def _same_bits(a, b):
    xa, xb = _bits(a), _bits(b)
    assert len(xa) == len(xb)
    for x, y in zip(xa, xb):
        assert np.array_equal(x, y)


def _records(name, got, op):
    return [g for st, g in zip(seq.SEQUENCES[name][1], got) if st[0] == op]


def _run_one(name, before=None, counters=None):
    """SEQUENCES[name] on one fresh GPU problem of one rank; the problem is closed whatever happens.
    counters: (boundary_device, boundary_host) expected after the whole sequence"""
    from qsp_slam_amd.ba import BaProblem
    sname, steps = seq.SEQUENCES[name]
    sc = seq.scene(sname)
    p = BaProblem(sc)
    try:
        if before is not None:
            before(p)
        got = seq.run(p, sc, steps, _option())
        st = p.profile(False)
        if counters is not None:
            assert (st.boundary_device, st.boundary_host) == counters
        return got, st
    finally:
        p.close()


def _fresh(sname, steps):
    """`steps` on a fresh problem (the reference of the bit-equality claims)"""
    from qsp_slam_amd.ba import BaProblem
    sc = seq.scene(sname)
    p = BaProblem(sc)
    try:
        return seq.run(p, sc, steps, _option())
    finally:
        p.close()


# ---- one rank ------------------------------------------------------------------------------------------------------------------

def test_a_solve_after_a_device_boundary_runs_on_the_stage_two_outlier_set():
    """A: local_joint [device boundary] -> optimize(3, Huber) with no set_state and no set_levels in between.  The host's level
    arrays lag the device's pointer swap here; the third solve must linearise the stage-2 outlier set (on all-active levels its
    first chi2 would be off by orders of magnitude, tests/test_oracle_ba_sequences.py) and index() must be the oracle's."""
    got, _ = _run_one("A", counters=(1, 0))
    _against_oracle("A", got)


def test_b_edges_and_index_after_the_pointer_swap():
    """B: local_joint [device boundary] -> edges() -> index(): per-edge chi2 of the last evaluation that had the edge active, depth
    signs, and the index tables fetched lazily from the swapped device arrays.
    Measured (profiles/ba_reuse_margins.json): mono and object edges 1.4e-8 and 3.5e-11 of the 1e-7 bar, the stereo edges 8.8e-8.
    That one figure is a single edge of a weakly constrained landmark: after the thirteen LM iterations its position differs by
    4e-9 m between the two implementations (the estimates' own bar is 1e-7), and a single edge's chi2 follows the estimates to
    first order -- unlike the summed chi2 at the minimum, which agrees to 9e-12.  Both sides are bit-reproducible, so is the figure."""
    got, _ = _run_one("B", counters=(1, 0))
    _against_oracle("B", got)


def test_c_custom_levels_after_a_device_boundary_replace_the_outlier_set():
    """C: local_joint [device boundary] -> set_levels(every edge of landmark 0) -> optimize(2): the stale host copy must not come
    back, the stage-2 outliers are active again and landmark 0 leaves the index"""
    got, _ = _run_one("C", counters=(1, 0))
    _against_oracle("C", got)
    t = _records("C", got, "optimize")[0]["t"]
    assert t["pt_hidx"][0] == -1 and (t["pt_hidx"] >= 0).sum() == t["n_landmarks"]


def test_d_host_boundary_twice_on_one_problem():
    """D: local_joint [host boundary: object 0 leaves the index] -> set_state(initial) -> local_joint: the second run starts from
    the all-active index with object 0 back in it, takes the host path again and repeats the first bit for bit"""
    got, _ = _run_one("D", counters=(0, 2))
    _against_oracle("D", got)
    first, second = _records("D", got, "local_joint")
    _same_bits(first, second)
    assert first["t1"]["n_pose_blocks"] == first["t2"]["n_pose_blocks"] + 1 == second["t1"]["n_pose_blocks"]      # object 0


def test_e_object_elimination_off_and_on_again_against_the_cached_index():
    """E: local_joint [device] -> set_object_elimination(False) -> set_state -> local_joint -> set_object_elimination(True) ->
    set_state -> local_joint.  The all-active index is cached per problem and carries whether the objects are eliminated; a cache
    that ignored the option would run the second solve in the first one's form.  n_pose_blocks (free key-frames + objects) does
    not depend on the option by its definition in include/qsp_hip.h, so the form is told by the bits: the second run equals a
    fresh problem with the elimination off and differs from the first, the third equals the first."""
    got, _ = _run_one("E", counters=(3, 0))
    _against_oracle("E", got)
    first, second, third = _records("E", got, "local_joint")
    _same_bits(first, third)
    joint = _fresh("device", [seq.ELIM_OFF, seq.LJ])[1]
    _same_bits(second, joint)
    assert not all(np.array_equal(x, y) for x, y in zip(_bits(first), _bits(second)))
    assert first["t1"]["n_pose_blocks"] == second["t1"]["n_pose_blocks"] == third["t1"]["n_pose_blocks"]


def test_f_all_active_levels_after_custom_levels_equal_a_fresh_problem():
    """F: set_levels(custom) -> optimize -> set_levels(None) -> set_state(initial) -> optimize, atomic-free mode: the deferred
    zeroing of the device levels and the all-active index built AFTER a custom one give the bits of a fresh problem"""
    got, _ = _run_one("F")
    _against_oracle("F", got)
    last = _records("F", got, "optimize")[1]
    fresh = _fresh("sharded", [seq.DET_ON, seq.SEQUENCES["F"][1][-1]])[1]
    _same_bits(last, fresh)
    _same_index([last["t"][k] for k in ("kf_hidx", "obj_hidx", "pt_hidx")], [fresh["t"][k] for k in ("kf_hidx", "obj_hidx", "pt_hidx")])


def test_g_deterministic_mode_off_and_on_again():
    """G: atomic-free -> FP64 atomics -> atomic-free, set_state(initial) + local_joint each time: the first and third runs have
    the same bits, the atomic run in between holds the oracle's bars"""
    got, _ = _run_one("G", counters=(3, 0))
    _against_oracle("G", got)
    first, second, third = _records("G", got, "local_joint")
    _same_bits(first, third)


def test_h_a_stopped_local_joint_leaves_the_problem_as_it_was():
    """H: local_joint with the stop flag up returns with estimates, levels and counters untouched; the next local_joint equals a
    fresh problem's"""
    got, st = _run_one("H")
    _against_oracle("H", got)
    sc = seq.scene("sharded")
    for a, b in zip(_records("H", got, "local_joint_stopped")[0]["state"], (sc["kf_pose"], sc["pt_xyz"], sc["obj_pose"])):
        assert np.array_equal(a, b)
    assert st.boundary_device + st.boundary_host == 1
    _same_bits(_records("H", got, "local_joint")[0], _fresh("sharded", [seq.LJ])[0])


def test_i_step_form_of_the_factorisation_on_a_problem_that_ran_the_chain():
    """I: local_joint [device, chain form] -> set_cholesky_chain(False) -> set_state -> local_joint: same operations in the same
    order, same bits; no flag wait expired on the way"""
    def chain_is_on(p):
        if not p.cholesky_chain:
            pytest.fail("the chain form was not set up for a problem with several block rows")
    got, st = _run_one("I", before=chain_is_on, counters=(2, 0))
    _against_oracle("I", got)
    first, second = _records("I", got, "local_joint")
    _same_bits(first, second)
    assert st.chain_timeouts == 0 and not st.cholesky_chain


# ---- two ranks: threads on the one GPU, host-summed all-reduce hook ----------------------------------------------------------------

def _run_two_ranks(name):
    """SEQUENCES[name] on two problems, one per thread, in the pattern of test_landmark_sharded_ba_equals_single_rank.  Returns
    (records per rank, boundary counters per rank after the steps before the first set_shard).  Every problem is closed."""
    from qsp_slam_amd.ba import BaProblem
    from qsp_slam_amd.parallel import ThreadAllreduce
    sname, steps = seq.SEQUENCES[name]
    sc = seq.scene(sname)
    world = 2
    comm = ThreadAllreduce(world)
    first_shard = [s[0] for s in steps].index("set_shard")
    out, counters, err = [None] * world, [None] * world, []

    def run(rank):
        p = None
        try:
            p = BaProblem(sc)
            got = seq.run(p, sc, steps[:first_shard], _option(rank, comm))
            st = p.profile(False)
            counters[rank] = (st.boundary_device, st.boundary_host)
            got += seq.run(p, sc, steps[first_shard:], _option(rank, comm))
            out[rank] = got
        except Exception as e:      # pragma: no cover
            err.append(e)
            comm.barrier.abort()
        finally:
            if p is not None:
                p.close()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=100)
    if any(t.is_alive() for t in th):      # pragma: no cover (a rank left alone at the barrier: let it go, then fail)
        comm.barrier.abort()
        for t in th:
            t.join(timeout=10)
        err.append(RuntimeError("the ranks did not finish together"))
    assert not err, err
    return out, counters


@pytest.mark.timeout(120)
def test_s1_sharding_after_set_levels_none_keeps_the_ownership_mask():
    """S1: set_levels(None) -> set_shard(r, 2) -> optimize(4, Huber).  The zeroing that set_levels(None) leaves to the next solve
    must not wipe the mask set_shard wrote in between: every rank would linearise every edge and the summed chi2 double."""
    out, _ = _run_two_ranks("S1")
    for rank in range(2):
        _against_oracle("S1", out[rank])


@pytest.mark.timeout(120)
def test_s2_sharding_after_a_device_boundary_keeps_the_outlier_set_and_hides_the_mask():
    """S2: one rank's local_joint [device boundary, asserted] -> set_shard(r, 2) -> optimize(3, Huber) -> index().  The stage-2
    levels live on the device only when set_shard arrives; they must reach the sharded solve, and no landmark may be missing from
    index() because another rank owns it."""
    out, counters = _run_two_ranks("S2")
    assert counters == [(1, 0), (1, 0)]
    for rank in range(2):
        _against_oracle("S2", out[rank])


@pytest.mark.timeout(120)
def test_s3_resharding_to_the_other_rank_after_a_sharded_local_joint():
    """S3: set_shard(r, 2) -> local_joint -> index() -> set_shard(1 - r, 2) -> optimize(3, Huber) -> index(): the mask never survives a
    change of (rank, world), the outlier set does"""
    out, _ = _run_two_ranks("S3")
    for rank in range(2):
        _against_oracle("S3", out[rank])


@pytest.mark.timeout(120)
def test_s4_unsharding_gives_back_a_single_rank_problem():
    """S4: set_shard(r, 2) -> local_joint -> set_shard(0, 1) -> atomic-free mode -> set_state(initial) -> local_joint.  The two
    ranks' last runs are unsharded and independent; rank 0's is compared, to the bit, with a fresh unsharded problem"""
    out, _ = _run_two_ranks("S4")
    for rank in range(2):
        _against_oracle("S4", out[rank])
    fresh = _fresh("sharded", [seq.DET_ON, seq.LJ])[1]
    for rank in range(2):
        _same_bits(_records("S4", out[rank], "local_joint")[1], fresh)
