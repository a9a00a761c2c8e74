"""GPU parity tests of hot path B (joint bundle adjustment) through the C-ABI, against the C oracle (oracle/ba_oracle.c,
itself pinned by an independent dense formulation in tests/test_oracle_ba.py) run live on the same seeded scenes, and
against committed fixtures of the oracle's output (tests/golden/ba_*.npz).

Bars: hessian indices, trial counts, accept flags and outlier levels bit-exact; chi2 / lambda / estimates to 1e-8 relative
(FP64 on both sides; differences come only from summation order and the Cholesky variant) -- far inside the 1e-4 pose bar.
The default Schur complement is atomic-free and bit-reproducible; the FP64-atomic kernels (large graphs, or
set_deterministic(False)) have a run-to-run spread of up to 7e-9 relative on the ill-conditioned 4-key-frame scene
(tools/ba_repeat.py) and are covered by test_atomic_schur_kernels_match_oracle and the large-graph test."""
import os

import numpy as np
import pytest

from oracle import ba_oracle as bo
from qsp_slam_amd import synth
from tests import ba_sequences as seq

pytestmark = pytest.mark.gpu

DM = float(np.float32(np.sqrt(5.991)))
DS = float(np.float32(np.sqrt(7.815)))
DO = float(np.float32(np.sqrt(1e3)))

SCENES = {
    "tiny": dict(seed=3, n_kf=4, n_pt=30, n_obj=1, stereo_frac=0.3, obs_per_obj=3),
    "mono": dict(seed=4, n_kf=8, n_pt=300, n_obj=3, stereo_frac=0.0),
    "stereo": dict(seed=5, n_kf=6, n_pt=150, n_obj=0, stereo_frac=1.0),
    "c1": dict(seed=31, n_kf=10, n_pt=1000, n_obj=2, stereo_frac=0.0),                  # BASELINE config 1 shape
    "c2": dict(seq.C2),                                                                 # BASELINE config 2 shape
    "two_fixed": dict(seed=6, n_kf=12, n_pt=500, n_obj=4, stereo_frac=0.5, n_fixed=3),
}


def close(a, b, rtol=1e-8, atol=1e-12):
    """np.allclose(a, b, rtol, atol), with the measured effective relative error max |a-b| / (|b| + atol/rtol) recorded under
    the calling test's name (tests/margins.py -> profiles/r02_test_margins.json)."""
    import inspect
    from tests.margins import within
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    f = inspect.stack()[1]
    test = os.environ.get("PYTEST_CURRENT_TEST", f.function).split("::")[-1].split(" ")[0]
    eff = float((np.abs(a - b) / (np.abs(b) + atol / rtol)).max()) if a.size else 0.0
    return within("ba/%s:%d" % (test, f.lineno), eff, rtol) and bool(np.isfinite(a).all())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_single_stage_matches_oracle(name):
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene(**SCENES[name])
    ref = bo.BaProblem(sc)
    tr = ref.optimize(6, DM, DS, DO)
    gpu = BaProblem(sc)
    tg = gpu.optimize(6, DM, DS, DO)
    # bit-exact index tables (g2o's buildIndexMapping order)
    assert np.array_equal(tg["kf_hidx"], tr["kf_hidx"])
    assert np.array_equal(tg["obj_hidx"], tr["obj_hidx"])
    assert np.array_equal(tg["pt_hidx"], tr["pt_hidx"])
    assert list(tg["trials"]) == list(tr["trials"]) and list(tg["accepted"]) == list(tr["accepted"])
    assert tg["result"] == tr["result"] and tg["iterations"] == tr["iterations"]
    assert close(tg["chi2"], tr["chi2"]) and close(tg["lam"], tr["lam"])
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert close(kf, rkf, rtol=1e-8, atol=1e-10) and close(pt, rpt, rtol=1e-8, atol=1e-10)
    if len(rob):
        assert close(ob, rob, rtol=1e-8, atol=1e-10)
    e = gpu.edges()
    assert close(e["mono_chi2"], ref.s["mono_chi2"][: ref.nm], rtol=1e-7, atol=1e-9)
    assert close(e["st_chi2"], ref.s["st_chi2"][: ref.ns], rtol=1e-7, atol=1e-9)
    assert close(e["oe_chi2"], ref.s["oe_chi2"][: ref.no], rtol=1e-7, atol=1e-9)
    gpu.close()


@pytest.mark.parametrize("mode", ["deterministic", "atomic"])
def test_landmarks_with_more_than_256_observations(mode):
    """260 key-frames, every landmark observed by all of them (> 256 edges per landmark): the landmark pass walks such a landmark
    in windows of 256 edges; before, qsp_ba_create refused the scene (and the drop-in Optimizer fell back to g2o)"""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene_large(11, 260, 60, obs_per_pt=260)
    ref = bo.BaProblem(sc)
    tr = ref.optimize(2, 0.0, 0.0, 0.0)
    gpu = BaProblem(sc)
    gpu.set_deterministic(mode == "deterministic")
    tg = gpu.optimize(2, 0.0, 0.0, 0.0)
    assert np.array_equal(tg["kf_hidx"], tr["kf_hidx"]) and np.array_equal(tg["pt_hidx"], tr["pt_hidx"])
    assert list(tg["trials"]) == list(tr["trials"]) and list(tg["accepted"]) == list(tr["accepted"])
    assert close(tg["chi2"], tr["chi2"], rtol=1e-8) and close(tg["lam"], tr["lam"], rtol=1e-8)
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert close(kf, rkf, rtol=1e-7, atol=1e-9) and close(pt, rpt, rtol=1e-7, atol=1e-9)
    gpu.close()


@pytest.mark.parametrize("name", ["tiny", "mono", "c2", "two_fixed"])
def test_local_joint_ba_two_stage_matches_oracle(name):
    """Optimizer::LocalJointBundleAdjustment schedule: same outlier set, same LM path, same estimates"""
    from qsp_slam_amd.ba import BaProblem
    kw = dict(SCENES[name], outlier_frac=0.08)
    sc = synth.make_ba_scene(**kw)
    ref = bo.BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    gpu = BaProblem(sc)
    g1, g2 = gpu.local_joint_ba()
    # the 4-key-frame scene with outliers is ill-conditioned: any re-association of the sums (oracle vs GPU) is amplified
    # to ~1e-8 relative in the final chi2 there (the atomic kernels' own run-to-run spread is 7e-9, tools/ba_repeat.py)
    tol = 1e-6 if name == "tiny" else 1e-8
    for g, r in ((g1, r1), (g2, r2)):
        assert list(g["trials"]) == list(r["trials"]) and list(g["accepted"]) == list(r["accepted"])
        assert close(g["chi2"], r["chi2"], rtol=tol) and close(g["lam"], r["lam"], rtol=tol)
        assert g["result"] == r["result"]
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    etol = 1e-5 if name == "tiny" else 1e-7
    assert close(kf, rkf, rtol=etol, atol=1e-9) and close(pt, rpt, rtol=etol, atol=1e-9) and close(ob, rob, rtol=etol, atol=1e-9)
    # pose bar of north_star: 1e-4 relative -- met with a wide margin
    assert np.abs(kf - rkf).max() < 1e-4 * np.abs(rkf).max()
    # index tables of the second stage (outliers removed -> some points may drop out)
    kh, oh, ph = gpu.index()
    assert np.array_equal(kh, r2["kf_hidx"]) and np.array_equal(oh, r2["obj_hidx"]) and np.array_equal(ph, r2["pt_hidx"])
    gpu.close()


def test_stage_boundary_paths_device_and_host():
    """Round 4: the boundary between optimize(5) and optimize(10) of a local BA (outlier classification, re-index, the second
    stage's first system) runs on the device behind the first stage's last trial; it falls back to the host path when a pose
    vertex would leave the index.  Both are exercised and counted (qsp_ba_stats.boundary_device / boundary_host), both against
    the oracle, and both give the same bits as the host path forced from the start (QSP_BA_HOST_BOUNDARY is read once per process,
    so the comparison here is device path vs oracle + a second run of the same problem: bit-reproducible)."""
    from qsp_slam_amd.ba import BaProblem
    # (1) an ordinary scene: device path
    sc = synth.make_ba_scene(**dict(SCENES["c2"], outlier_frac=0.08))
    ref = bo.BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    gpu = BaProblem(sc)
    g1, g2 = gpu.local_joint_ba()
    st = gpu.profile(False)
    assert (st.boundary_device, st.boundary_host) == (1, 0)
    assert list(g2["trials"]) == list(r2["trials"]) and close(g2["chi2"], r2["chi2"], rtol=1e-8)
    kh, oh, ph = gpu.index()                      # (fetched lazily from the device after the pointer swap)
    assert np.array_equal(kh, r2["kf_hidx"]) and np.array_equal(oh, r2["obj_hidx"]) and np.array_equal(ph, r2["pt_hidx"])
    assert (ph < 0).sum() == (r2["pt_hidx"] < 0).sum()
    first = (np.array(g2["chi2"]), *gpu.state())
    gpu.set_state(sc["kf_pose"], sc["pt_xyz"], sc["obj_pose"])      # the same problem again: cached all-active index, level reset in
    h1, h2 = gpu.local_joint_ba()                                   # k_edge_index, second buffers swapped back
    assert gpu.profile(False).boundary_device == 2
    for x, y in zip((np.array(h2["chi2"]), *gpu.state()), first):
        assert np.array_equal(x, y)
    gpu.close()
    # (2) one object's camera-object measurements are mutually inconsistent (each off by metres in its own direction): after the
    # first stage every one of its edges is an outlier, the object vertex leaves the index, the reduced system shrinks -> host path
    sc2 = seq.host_boundary_scene()
    ref = bo.BaProblem(sc2)
    r1, r2 = ref.local_joint_ba()
    assert r2["obj_hidx"][0] < 0 and (r2["obj_hidx"][1:] >= 0).all()           # the oracle drops object 0 from the second stage
    gpu = BaProblem(sc2)
    g1, g2 = gpu.local_joint_ba()
    st = gpu.profile(False)
    assert (st.boundary_device, st.boundary_host) == (0, 1)
    for g, r in ((g1, r1), (g2, r2)):
        assert list(g["trials"]) == list(r["trials"]) and close(g["chi2"], r["chi2"], rtol=1e-8)
    kh, oh, ph = gpu.index()
    assert np.array_equal(kh, r2["kf_hidx"]) and np.array_equal(oh, r2["obj_hidx"]) and np.array_equal(ph, r2["pt_hidx"])
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert close(kf, rkf, rtol=1e-7, atol=1e-9) and close(pt, rpt, rtol=1e-7, atol=1e-9) and close(ob, rob, rtol=1e-7, atol=1e-9)
    gpu.close()


def test_against_committed_fixture(golden_dir):
    from qsp_slam_amd.ba import BaProblem
    z = np.load(os.path.join(golden_dir, "ba_local_joint_c1.npz"))
    sc = synth.make_ba_scene(**SCENES["c1"], outlier_frac=0.05)
    assert np.array_equal(sc["mono_obs"], z["mono_obs"])          # the generator is still byte-stable
    gpu = BaProblem(sc)
    g1, g2 = gpu.local_joint_ba()
    assert close(g1["chi2"], z["chi2_1"], rtol=1e-8) and close(g2["chi2"], z["chi2_2"], rtol=1e-8)
    assert list(g1["trials"]) == list(z["trials_1"]) and list(g2["trials"]) == list(z["trials_2"])
    kf, pt, ob = gpu.state()
    assert close(kf, z["kf"], rtol=1e-7, atol=1e-9) and close(pt, z["pt"], rtol=1e-7, atol=1e-9)
    assert close(ob, z["ob"], rtol=1e-7, atol=1e-9)
    kh, oh, ph = gpu.index()
    assert np.array_equal(kh, z["kf_hidx"]) and np.array_equal(ph, z["pt_hidx"])
    gpu.close()


def test_stop_flag_and_levels():
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene(13, 5, 60, 1)
    gpu = BaProblem(sc)
    before = gpu.state()
    t = gpu.optimize(5, DM, DS, DO, stop=np.ones(1, np.uint8))
    assert t["iterations"] == 0 and t["result"] == 2
    assert all(np.array_equal(a, b) for a, b in zip(before, gpu.state()))
    # excluding every edge of one point removes it from the index (hessian index -1), as g2o's active-vertex rule does
    lv = (sc["mono_pt"] == 0).astype(np.uint8)
    gpu.set_levels(mono=lv)
    ref = bo.BaProblem(sc)
    ref.s["mono_level"][: ref.nm] = lv
    tg, tr = gpu.optimize(2, 0, 0, 0), ref.optimize(2, 0, 0, 0)
    assert tg["pt_hidx"][0] == -1 and np.array_equal(tg["pt_hidx"], tr["pt_hidx"])
    assert close(tg["chi2"], tr["chi2"])
    gpu.close()


def test_points_only_bundle_adjustment_no_objects():
    """Optimizer::LocalBundleAdjustment (src/Optimizer.cc:458-783) is the same graph without object vertices"""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene(41, 10, 400, 0, stereo_frac=0.3)
    ref, gpu = bo.BaProblem(sc), BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    g1, g2 = gpu.local_joint_ba()
    assert close(g2["chi2"], r2["chi2"], rtol=1e-8)
    assert close(gpu.state()[0], ref.state()[0], rtol=1e-7, atol=1e-9)
    gpu.close()


@pytest.mark.parametrize("world", [2, 3])
def test_landmark_sharded_ba_equals_single_rank(world):
    """qsp_ba_set_shard: `world` shards of one scene (here: threads on the one GPU, host-summed all-reduce hook) walk the
    same Levenberg-Marquardt path and end in the same state as the unsharded solve.  Sums are re-associated across
    ranks, so agreement is to ~1e-9, not bit-exact."""
    import threading
    from qsp_slam_amd.ba import BaProblem
    from qsp_slam_amd.parallel import ThreadAllreduce
    sc = synth.make_ba_scene(seed=61, n_kf=10, n_pt=400, n_obj=3, stereo_frac=0.3, outlier_frac=0.06)
    ref = BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    rkf, rpt, rob = ref.state()
    comm = ThreadAllreduce(world)
    out, err = [None] * world, []

    def run(rank):
        try:
            p = BaProblem(sc)
            p.set_shard(rank, world, comm.hook(rank))
            t1, t2 = p.local_joint_ba()
            out[rank] = (t1, t2, p.state(), p.index())
            p.close()
        except Exception as e:      # pragma: no cover
            err.append(e)
            comm.barrier.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not err, err
    for rank in range(world):
        t1, t2, (kf, pt, ob), (kh, oh, ph) = out[rank]
        assert list(t1["trials"]) == list(r1["trials"]) and list(t2["trials"]) == list(r2["trials"])
        assert close(t1["chi2"], r1["chi2"], rtol=1e-8) and close(t2["chi2"], r2["chi2"], rtol=1e-8)
        assert close(t1["lam"], r1["lam"], rtol=1e-7)
        assert close(kf, rkf, rtol=1e-7, atol=1e-9) and close(pt, rpt, rtol=1e-7, atol=1e-9) and close(ob, rob, rtol=1e-7, atol=1e-9)
        assert np.array_equal(kh, ref.index()[0]) and np.array_equal(ph, ref.index()[2])
    ref.close()


def test_sharded_ba_with_rccl_world_of_one():
    """the production hook (torch.distributed all_reduce on RCCL) on a 1-rank group: exercises the device-pointer view and
    the stream hand-over; world == 1 short-circuits inside the library, so the hook is also called directly"""
    import torch
    import torch.distributed as dist
    from qsp_slam_amd.ba import BaProblem
    from qsp_slam_amd.parallel import TorchAllreduce
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        hook = TorchAllreduce(0)
        x = torch.arange(8, dtype=torch.float64, device="cuda:0")
        hook(x.data_ptr(), 8, 0)                       # sum over one rank = identity
        assert torch.equal(x.cpu(), torch.arange(8, dtype=torch.float64))
        sc = synth.make_ba_scene(seed=62, n_kf=5, n_pt=80, n_obj=1)
        p = BaProblem(sc)
        p.set_shard(0, 1, hook)
        t1, t2 = p.local_joint_ba()
        assert t2["chi2"][-1] < t1["chi2"][0]
        p.close()
    finally:
        dist.destroy_process_group()


def test_library_rccl_communicator_world_of_one():
    """qsp_comm_* + qsp_ba_set_shard_rccl on a 1-rank communicator: librccl resolves at run time, the collectives run on the
    library's stream (sum over one rank = identity), world == 1 leaves the solve unsharded and bit-identical"""
    import ctypes
    from qsp_slam_amd import parallel
    from qsp_slam_amd.ba import BaProblem
    c = parallel.RcclComm(0, 1, 0)
    assert c.nccl()
    hip = parallel._hip()
    buf = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(buf), 8 * 16) == 0
    host = np.arange(16, dtype=np.float64)
    hip.hipMemcpy(buf, host.ctypes.data_as(ctypes.c_void_p), 128, 1)
    c.allreduce_f64(buf.value, 16)
    hip.hipDeviceSynchronize()
    back = np.zeros(16)
    hip.hipMemcpy(back.ctypes.data_as(ctypes.c_void_p), buf, 128, 2)
    hip.hipFree(buf)
    assert np.array_equal(back, host)
    sc = synth.make_ba_scene(seed=62, n_kf=5, n_pt=80, n_obj=1)
    a, b = BaProblem(sc), BaProblem(sc)
    b.set_shard_rccl(c)
    ta, tb = a.local_joint_ba(), b.local_joint_ba()
    assert np.array_equal(ta[1]["chi2"], tb[1]["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    a.close()
    b.close()
    c.close()


@pytest.mark.parametrize("mode", ["deterministic", "atomic"])
def test_block_row_schur_path_on_a_large_graph(mode):
    """80 000 edges (12 key-frames, 10 000 landmarks x 8 observations, 2 objects), against the C oracle on the same graph with the
    bars of the small scenes.  The graph holds 360 000 pair entries, far under the cap, so its default mode is the pair lists
    (`deterministic`: k_schur_pairs, form 0); only in the atomic mode do >= 65536 edges switch the Schur complement to
    k_schur_rows (LDS row blocks per key-frame split, form 2).  qsp_ba_stats.schur_form is the witness of which one ran."""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene_large(11, 12, 10000, obs_per_pt=8, n_obj=2)
    assert len(sc["mono_pt"]) >= 65536
    ref = bo.BaProblem(sc)
    tr = ref.optimize(4, DM, DS, DO)
    gpu = BaProblem(sc)
    if mode == "atomic":
        gpu.set_deterministic(False)
    tg = gpu.optimize(4, DM, DS, DO)
    assert gpu.schur_form == (0 if mode == "deterministic" else 2)
    assert np.array_equal(tg["kf_hidx"], tr["kf_hidx"]) and np.array_equal(tg["pt_hidx"], tr["pt_hidx"])
    assert list(tg["trials"]) == list(tr["trials"]) and list(tg["accepted"]) == list(tr["accepted"])
    assert close(tg["chi2"], tr["chi2"]) and close(tg["lam"], tr["lam"])
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert close(kf, rkf, rtol=1e-8, atol=1e-10) and close(pt, rpt, rtol=1e-8, atol=1e-10)
    assert close(ob, rob, rtol=1e-8, atol=1e-10)
    gpu.close()


@pytest.mark.parametrize("name", ["tiny", "mono", "c2", "two_fixed"])
def test_deterministic_mode_is_bit_reproducible_and_matches_oracle(name):
    """qsp_ba_set_deterministic: the Schur complement without atomics.  Five runs give the same bits; against the oracle
    the well-posed scenes hold 1e-9 (the ill-conditioned 4-key-frame scene 1e-6: there any re-association of the sums --
    oracle vs GPU -- is amplified the same way as the atomics' run-to-run noise)."""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene(**dict(SCENES[name], outlier_frac=0.08))
    ref = bo.BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    runs = []
    for _ in range(5):
        gpu = BaProblem(sc)
        gpu.set_deterministic(True)
        g1, g2 = gpu.local_joint_ba()
        runs.append((np.array(g1["chi2"]), np.array(g2["chi2"]), np.array(g2["lam"]), *gpu.state()))
        gpu.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    tol = 1e-6 if name == "tiny" else 1e-9
    assert list(g1["trials"]) == list(r1["trials"]) and list(g2["trials"]) == list(r2["trials"])
    assert close(g1["chi2"], r1["chi2"], rtol=tol) and close(g2["chi2"], r2["chi2"], rtol=tol)
    rkf, rpt, rob = ref.state()
    etol = 1e-5 if name == "tiny" else 1e-7
    assert close(runs[0][3], rkf, rtol=etol, atol=1e-9) and close(runs[0][4], rpt, rtol=etol, atol=1e-9)


def test_deterministic_mode_full_size_c4_and_sharded_consistency():
    """C4-size graph: deterministic and default modes agree (1e-8), and the deterministic mode repeats bit-exactly"""
    import bench
    from qsp_slam_amd.ba import BaProblem
    w = bench.WORKLOADS["c4"]
    sc = synth.make_ba_scene(2000, w["n_kf"], w["n_map"], w["n_obj"], stereo_frac=0.2)
    a = BaProblem(sc)
    a1, a2 = a.local_joint_ba()
    ka, pa, oa = a.state()
    a.close()
    outs = []
    for _ in range(2):
        b = BaProblem(sc)
        b.set_deterministic(True)
        b1, b2 = b.local_joint_ba()
        outs.append((np.array(b2["chi2"]), *b.state()))
        b.close()
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x, y)
    assert list(b2["trials"]) == list(a2["trials"])
    assert np.allclose(outs[0][0], a2["chi2"], rtol=1e-8)
    assert np.allclose(outs[0][1], ka, rtol=1e-7, atol=1e-10) and np.allclose(outs[0][2], pa, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("size", ["c2", "c4", "c5"])
def test_cholesky_chain_and_step_forms_give_the_same_bits(size):
    """QSP_BA_OPT_CHOLESKY_CHAIN: the factorisation as one launch (a resident chain workgroup + tile workgroups that take
    tickets, k_chol_solve) against one launch per block step (2, 5 and 19 block rows): the same operations in the same order, so
    the whole two-stage BA -- chi2 and lambda per iteration, trials, final poses and points -- is identical to the bit.  The
    chain form must be the one in use (a silent fall-back to the step form would make this test vacuous).  The other block counts
    (1, 2, 3, 4, 6, 18, the first with a second ticket per tile workgroup, 31 and 32), each also against the oracle:
    tests/test_gpu_ba_blocks.py."""
    import bench
    from qsp_slam_amd.ba import BaProblem
    w = bench.WORKLOADS[size]
    sc = synth.make_ba_scene(2100, w["n_kf"], w["n_map"], w["n_obj"], stereo_frac=0.2)
    outs = []
    for chain in (True, False):
        b = BaProblem(sc)
        b.set_deterministic(True)
        if chain:
            if not b.cholesky_chain:
                b.close()
                pytest.fail("the chain form was not set up for a problem with several block rows")
        else:
            b.set_cholesky_chain(False)
        assert b.cholesky_chain == chain
        b1, b2 = b.local_joint_ba()
        if chain:       # no flag wait expired: the problem is still on the chain form (a time-out would cost 1-2 s, not the result)
            assert b.profile(False).chain_timeouts == 0 and b.cholesky_chain
        outs.append((np.array(b1["chi2"]), np.array(b1["lam"]), np.array(b2["chi2"]), np.array(b2["lam"]), list(b1["trials"]) + list(b2["trials"]),
                     *b.state()))
        b.close()
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_destroyed_problems_leave_their_buffers_for_the_next_and_release_gives_them_back():
    """qsp_ba_destroy caches streams / device chunks / pinned buffers per device (the drop-in Optimizer builds a problem per
    call); results do not depend on what a recycled buffer held, and qsp_ba_release_caches returns the memory"""
    import ctypes as C
    from qsp_slam_amd import ba as gba
    from qsp_slam_amd.ba import BaProblem
    hip = C.CDLL("libamdhip64.so")

    def free_mb():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value / 2 ** 20

    big = synth.make_ba_scene(**SCENES["c2"])
    small = synth.make_ba_scene(**SCENES["mono"])
    gba.release_caches()
    outs = []
    for sc in (big, small, big, small, big):       # (recycled chunks hold the other scene's data)
        b = BaProblem(sc)
        b.set_deterministic(True)
        t1, t2 = b.local_joint_ba()
        outs.append((np.array(t2["chi2"]), b.state()[0]))
        b.close()
    assert np.array_equal(outs[0][0], outs[2][0]) and np.array_equal(outs[0][0], outs[4][0]) and np.array_equal(outs[1][0], outs[3][0])
    assert np.array_equal(outs[0][1], outs[4][1]) and np.array_equal(outs[1][1], outs[3][1])
    held = free_mb()
    gba.release_caches()
    assert free_mb() >= held + 7.5                 # (at least the 8 MB chunk of the last problem came back)


@pytest.mark.timeout(300)
def test_chain_factorisation_beside_a_decoder_that_fills_the_chip(golden_dir):
    """LocalMapping's bundle adjustment and object refinement run on different threads in the reference's system.  The decoder's
    kernels are persistent-style grids that hold every compute unit for tens of milliseconds; the BA's chain workgroup and its
    tile workgroups have to find their compute units in between and must neither starve into a wait time-out nor change a bit."""
    import threading
    import bench
    from qsp_slam_amd import DeepSdfDecoder
    from qsp_slam_amd.ba import BaProblem
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, RefineBatch, _joint_cfg
    from tests.test_gpu_sdf import make_cfg
    from oracle import sdf_oracle as so
    w = bench.WORKLOADS["c4"]
    sc = synth.make_ba_scene(2100, w["n_kf"], w["n_map"], w["n_obj"], stereo_frac=0.2)
    ref = BaProblem(sc)
    ref.set_deterministic(True)
    if not ref.cholesky_chain:
        ref.close()
        pytest.fail("the chain form was not set up for a problem with several block rows")
    r1, r2 = ref.local_joint_ba()
    want = (np.array(r2["chi2"]), *ref.state())
    ref.close()
    dec = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz"))
    dec.set_precision("fp16x2")
    opt = Optimizer(dec, make_cfg(so.JointConfig(n_iter=2)))
    objs = synth.make_object_views(77, 16, 4000, n_fg=256, n_bg=200)
    T0, hyp = bench.flip_states(objs, 4)
    batch = RefineBatch(dec, _joint_cfg(opt), [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs], hyp)
    stop = threading.Event()
    errors = []

    def load():
        try:
            while not stop.is_set():
                batch.set_state(T0, None)
                batch.run(2)
        except Exception as e:      # noqa: BLE001 (reported below)
            errors.append(e)

    th = threading.Thread(target=load)
    th.start()
    try:
        for _ in range(12):
            b = BaProblem(sc)
            b.set_deterministic(True)
            g1, g2 = b.local_joint_ba()
            got = (np.array(g2["chi2"]), *b.state())
            b.close()
            for x, y in zip(got, want):
                assert np.array_equal(x, y)
    finally:
        stop.set()
        th.join()
        batch.close()
        dec.close()
    assert not errors, errors


@pytest.mark.timeout(120)
def test_cholesky_chain_waits_are_bounded_and_an_expired_one_costs_time_not_the_solve():
    """ADVICE r3.  The chain workgroup launched without its tile workgroups (option value 2): the flag it waits for never comes,
    the wait expires after ~1e6 polls, later waits give up at once and the launch drains -- no hang.  The library then repeats
    THAT trial on the one-launch-per-step form from the backed-up estimates and keeps the problem on it: the call succeeds, every
    bit equals a problem that ran the step form from the start, the event is counted (qsp_ba_stats.chain_timeouts) and the
    problem stays usable."""
    import time
    import bench
    from qsp_slam_amd import _lib
    from qsp_slam_amd.ba import BaProblem
    w = bench.WORKLOADS["c4"]
    sc = synth.make_ba_scene(2100, w["n_kf"], w["n_map"], w["n_obj"], stereo_frac=0.2)
    ref = BaProblem(sc)
    ref.set_deterministic(True)
    ref.set_cholesky_chain(False)
    r1, r2 = ref.local_joint_ba()
    want = (np.array(r1["chi2"]), np.array(r2["chi2"]), np.array(r2["lam"]), list(r1["trials"]) + list(r2["trials"]), *ref.state())
    ref.close()
    b = BaProblem(sc)
    b.set_deterministic(True)
    assert b.cholesky_chain
    _lib.check(_lib.lib().qsp_ba_set_option(b.handle, 2, 2))
    t0 = time.perf_counter()
    g1, g2 = b.local_joint_ba()
    assert time.perf_counter() - t0 < 60
    got = (np.array(g1["chi2"]), np.array(g2["chi2"]), np.array(g2["lam"]), list(g1["trials"]) + list(g2["trials"]), *b.state())
    for x, y in zip(got, want):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert b.profile(False).chain_timeouts == 1 and not b.cholesky_chain
    b.set_state(sc["kf_pose"], sc["pt_xyz"], sc["obj_pose"])          # ... and the problem is still usable (on the step form)
    h1, h2 = b.local_joint_ba()
    assert np.array_equal(np.array(h2["chi2"]), want[1]) and b.profile(False).chain_timeouts == 1
    b.close()


@pytest.mark.parametrize("name", ["mono", "c2", "two_fixed"])
def test_atomic_schur_kernels_match_oracle(name):
    """set_deterministic(False): the per-landmark kernel with FP64 atomics (what graphs beyond the pair-list cap use
    together with the block-row kernel)"""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene(**dict(SCENES[name], outlier_frac=0.08))
    ref = bo.BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    gpu = BaProblem(sc)
    gpu.set_deterministic(False)
    g1, g2 = gpu.local_joint_ba()
    for g, r in ((g1, r1), (g2, r2)):
        assert list(g["trials"]) == list(r["trials"]) and list(g["accepted"]) == list(r["accepted"])
        assert close(g["chi2"], r["chi2"], rtol=1e-8) and close(g["lam"], r["lam"], rtol=1e-8)
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert close(kf, rkf, rtol=1e-7, atol=1e-9) and close(pt, rpt, rtol=1e-7, atol=1e-9)
    gpu.close()


@pytest.mark.parametrize("name", ["c2", "two_fixed", "tiny"])
def test_object_elimination_equals_joint_factorisation(name):
    """the second Schur complement over the (block-diagonal) object part == objects inside the dense system: same LM path,
    chi2 / estimates to rounding, and bit-reproducible; both against the oracle"""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene(**SCENES[name])
    ref = bo.BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    runs = []
    for elim in (True, True, False):
        g = BaProblem(sc)
        g.set_object_elimination(elim)
        t1, t2 = g.local_joint_ba()
        runs.append((t1, t2, g.state()))
        g.close()
    (a1, a2, sa), (b1, b2, sb), (c1, c2, sc_) = runs
    assert np.array_equal(a2["chi2"], b2["chi2"]) and all(np.array_equal(x, y) for x, y in zip(sa, sb))     # reproducible
    assert a1["n_pose_blocks"] == c1["n_pose_blocks"]
    for t, u in ((a1, c1), (a2, c2)):
        assert list(t["trials"]) == list(u["trials"]) and list(t["accepted"]) == list(u["accepted"])
        assert close(t["chi2"], u["chi2"], rtol=1e-8 if name != "tiny" else 1e-6)
    tol = 1e-7 if name != "tiny" else 1e-5
    for x, y in zip(sa, sc_):
        assert close(x, y, rtol=tol, atol=1e-9)
    for x, y in zip(sa, ref.state()):
        assert close(x, y, rtol=tol, atol=1e-9)
    assert close(a2["chi2"], r2["chi2"], rtol=1e-8 if name != "tiny" else 1e-6)


def test_objects_with_smaller_vertex_ids_than_keyframes_stay_in_the_dense_system():
    """the elimination needs every free key-frame in front of every object in g2o's hessian order; a caller with another id
    scheme gets the joint factorisation and the same answer as the oracle"""
    from qsp_slam_amd.ba import BaProblem
    sc = dict(synth.make_ba_scene(seed=71, n_kf=6, n_pt=120, n_obj=2))
    sc["obj_id"] = np.array([2, 4], np.int64)            # interleaved with the key-frame ids 0..5
    sc["kf_id"] = np.array([0, 1, 3, 5, 6, 7], np.int64)
    ref, gpu = bo.BaProblem(sc), BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    g1, g2 = gpu.local_joint_ba()
    kh, oh, ph = gpu.index()
    assert np.array_equal(kh, r2["kf_hidx"]) and np.array_equal(oh, r2["obj_hidx"]) and oh.min() < kh.max()
    assert list(g2["trials"]) == list(r2["trials"]) and close(g2["chi2"], r2["chi2"], rtol=1e-8)
    for x, y in zip(gpu.state(), ref.state()):
        assert close(x, y, rtol=1e-7, atol=1e-9)
    gpu.close()


def _thinned(sc, lonely_kf=5, single_obs_pt=7, unobserved_pt=9):
    """the scene with one free key-frame that observes nothing, one landmark seen exactly once (a rank-2 3x3 block that only
    the damping makes invertible) and one landmark no edge touches"""
    sc = dict(sc)

    def drop(prefix, mask):
        for k in list(sc):
            if k.startswith(prefix + "_") and hasattr(sc[k], "shape"):
                sc[k] = sc[k][~mask]
    for pre in ("mono", "st"):
        kf, pt = sc[pre + "_kf"], sc[pre + "_pt"]
        m = (kf == lonely_kf) | (pt == unobserved_pt)
        seen = np.nonzero((pt == single_obs_pt) & ~m)[0]
        m[seen[1:] if pre == "mono" else seen] = True
        drop(pre, m)
    drop("oe", sc["oe_kf"] == lonely_kf)
    return sc


@pytest.mark.parametrize("mode", ["deterministic", "atomic"])
def test_vertices_without_edges_and_single_observation_landmarks(mode):
    """g2o keeps such vertices in the index mapping; their blocks are the damping alone (or rank deficient + damping) and the
    increments stay finite -- same index tables, trial sequence and estimates as the oracle"""
    from qsp_slam_amd.ba import BaProblem
    sc = _thinned(synth.make_ba_scene(seed=77, n_kf=8, n_pt=200, n_obj=2, stereo_frac=0.3))
    assert (sc["mono_pt"] == 7).sum() + (sc["st_pt"] == 7).sum() == 1
    assert not ((sc["mono_kf"] == 5).any() or (sc["st_kf"] == 5).any() or (sc["oe_kf"] == 5).any())
    ref, gpu = bo.BaProblem(sc), BaProblem(sc)
    gpu.set_deterministic(mode == "deterministic")
    r1, r2 = ref.local_joint_ba()
    g1, g2 = gpu.local_joint_ba()
    kh, oh, ph = gpu.index()
    assert np.array_equal(kh, r2["kf_hidx"]) and np.array_equal(oh, r2["obj_hidx"]) and np.array_equal(ph, r2["pt_hidx"])
    for g, r in ((g1, r1), (g2, r2)):
        assert list(g["trials"]) == list(r["trials"]) and list(g["accepted"]) == list(r["accepted"])
        # lambda's update factor is a cubic in rho = (chi2 - chi2_new) / scale: at the last steps chi2 moves by 1e-5 of itself,
        # so 1e-10 of chi2 is 1e-5 of rho (measured: up to 1e-3 in the last lambda with the atomic Schur kernels, whose sums
        # differ from run to run; 1e-9 while chi2 still moves) -- lambda is compared where the iteration still makes progress
        assert close(g["chi2"], r["chi2"], rtol=1e-8)
        c = np.asarray(r["chi2"], np.float64)
        moving = np.concatenate([[True], (c[:-1] - c[1:]) > 1e-3 * c[:-1]])      # iterations whose chi2 still moves by > 1e-3
        assert close(np.asarray(g["lam"])[moving], np.asarray(r["lam"])[moving], rtol=1e-6)
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert np.array_equal(kf[5], sc["kf_pose"][5]) or close(kf[5], rkf[5], rtol=1e-9, atol=1e-12)   # nothing pulls on it
    assert np.array_equal(pt[9], rpt[9])
    assert close(kf, rkf, rtol=1e-7, atol=1e-9) and close(pt, rpt, rtol=1e-7, atol=1e-9) and close(ob, rob, rtol=1e-7, atol=1e-9)
    gpu.close()


def test_pose_graph_of_key_frames_and_objects_without_landmarks():
    """no map point at all (n_pt = 0, no reprojection edge): only the camera-object edges remain; nothing of the landmark
    side may be launched with an empty grid"""
    from qsp_slam_amd.ba import BaProblem
    sc = dict(synth.make_ba_scene(seed=78, n_kf=6, n_pt=40, n_obj=3, stereo_frac=0.3, obs_per_obj=4))
    for pre in ("mono", "st"):
        for k in list(sc):
            if k.startswith(pre + "_") and hasattr(sc[k], "shape"):
                sc[k] = sc[k][:0]
    for k in ("pt_xyz", "pt_id", "gt_pt"):
        sc[k] = sc[k][:0]
    ref, gpu = bo.BaProblem(sc), BaProblem(sc)
    r1, r2 = ref.local_joint_ba()
    g1, g2 = gpu.local_joint_ba()
    assert list(g1["trials"]) == list(r1["trials"]) and list(g1["accepted"]) == list(r1["accepted"])
    # the second stage starts at the converged state of this small problem: chi2 moves by less than 1e-15 of itself, so whether
    # the tenth trial of its only iteration counts as a gain is decided by the last bit on either side
    assert list(g2["trials"]) == list(r2["trials"])
    assert close(g1["chi2"], r1["chi2"], rtol=1e-8) and close(g2["chi2"], r2["chi2"], rtol=1e-8)
    kf, pt, ob = gpu.state()
    rkf, rpt, rob = ref.state()
    assert pt.shape[0] == 0 and close(kf, rkf, rtol=1e-7, atol=1e-9) and close(ob, rob, rtol=1e-7, atol=1e-9)
    gpu.close()


@pytest.mark.parametrize("n_kf", [560, 620])
def test_many_keyframes_with_objects_in_the_atomic_mode(n_kf):
    """k_obj_rows, the atomic mode's object update, keeps a 6 x dimp row block in LDS (48 dimp bytes of 160 KB):
    beyond ~568 free key-frames it does not fit, and the launch used to be issued anyway (rejected, unchecked: Hs without the
    object terms).  Now build_index leaves the objects in the dense system above that size.  560 key-frames: the eliminated
    form at the edge of its LDS budget; 620: the guarded form.  Each against the atomic-free mode (pair lists, no LDS row
    blocks) on the same graph: same LM path, chi2 and estimates to rounding."""
    from qsp_slam_amd.ba import BaProblem
    sc = synth.make_ba_scene_large(17, n_kf, 4000, obs_per_pt=8, n_obj=3)
    runs = []
    for det in (False, True):
        g = BaProblem(sc)
        g.set_deterministic(det)
        t = g.optimize(2, DM, DS, DO)
        runs.append((t, g.state()))
        g.close()
    (ta, sa), (td, sd) = runs
    assert ta["n_pose_blocks"] == td["n_pose_blocks"] and ta["n_pose_blocks"] >= n_kf - 2 + 3
    assert list(ta["trials"]) == list(td["trials"]) and list(ta["accepted"]) == list(td["accepted"])
    assert close(ta["chi2"], td["chi2"], rtol=1e-8) and close(ta["lam"], td["lam"], rtol=1e-7)
    for x, y in zip(sa, sd):
        assert close(x, y, rtol=1e-7, atol=1e-9)
    assert float(ta["chi2"][-1]) < float(ta["chi2"][0]) or len(ta["chi2"]) == 1      # (and the step did reduce the cost)
