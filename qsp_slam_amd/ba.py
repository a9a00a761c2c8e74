"""Host-side handle of the joint bundle adjustment (path B) over the C-ABI of include/qsp_hip.h.

`scene` is the flattened g2o graph (see qsp_ba_scene in the header and qsp_slam_amd.synth.make_ba_scene): what
Optimizer::LocalJointBundleAdjustment / JointBundleAdjustment (src/Optimizer_util.cc) assemble from KeyFrame / MapPoint /
MapObject getters.  The C++ shim that does that flattening inside ORB-SLAM2 is include/qsp_optimizer_shim.h."""
import ctypes as C

import numpy as np

from . import _lib


def _arr(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a if a.size else np.zeros(8, dt)


class Trace(object):
    def __init__(self, cap):
        cap = max(int(cap), 1)
        self.chi2, self.lam = np.zeros(cap), np.zeros(cap)
        self.trials, self.accepted = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        self.c = _lib.BaTrace(cap, 0, _lib.dptr(self.chi2), _lib.dptr(self.lam), _lib.i32ptr(self.trials),
                              _lib.i32ptr(self.accepted), 0, 0, 0, 0)

    def dict(self):
        n = self.c.n
        return dict(iterations=self.c.iterations, chi2=self.chi2[:n].copy(), lam=self.lam[:n].copy(),
                    trials=self.trials[:n].copy(), accepted=self.accepted[:n].copy(), result=self.c.result,
                    n_pose_blocks=self.c.n_pose_blocks, n_landmarks=self.c.n_landmarks)


class BaProblem(object):
    def __init__(self, scene, device=0):
        L = _lib.lib()
        s = scene
        self.n_kf, self.n_pt, self.n_obj = len(s["kf_pose"]), len(s["pt_xyz"]), len(s["obj_pose"])
        self.nm, self.ns, self.no = len(s["mono_pt"]), len(s["st_pt"]), len(s["oe_kf"])
        k = self._keep = dict(
            kf_pose=_arr(s["kf_pose"], np.float64), kf_fixed=_arr(s["kf_fixed"], np.uint8),
            kf_id=_arr(s["kf_id"], np.int64), kf_K=_arr(s["kf_K"], np.float64), pt_xyz=_arr(s["pt_xyz"], np.float64),
            pt_id=_arr(s["pt_id"], np.int64), obj_pose=_arr(s["obj_pose"], np.float64),
            obj_id=_arr(s["obj_id"], np.int64), mono_pt=_arr(s["mono_pt"], np.int32), mono_kf=_arr(s["mono_kf"], np.int32),
            mono_obs=_arr(s["mono_obs"], np.float64), mono_info=_arr(s["mono_info"], np.float64),
            st_pt=_arr(s["st_pt"], np.int32), st_kf=_arr(s["st_kf"], np.int32), st_obs=_arr(s["st_obs"], np.float64),
            st_info=_arr(s["st_info"], np.float64), oe_kf=_arr(s["oe_kf"], np.int32), oe_obj=_arr(s["oe_obj"], np.int32),
            oe_meas=_arr(s["oe_meas"], np.float64))
        sc = _lib.BaScene(self.n_kf, self.n_pt, self.n_obj, self.nm, self.ns, self.no,
                          _lib.dptr(k["kf_pose"]), _lib.u8ptr(k["kf_fixed"]), _lib.i64ptr(k["kf_id"]),
                          _lib.dptr(k["kf_K"]), _lib.dptr(k["pt_xyz"]), _lib.i64ptr(k["pt_id"]),
                          _lib.dptr(k["obj_pose"]), _lib.i64ptr(k["obj_id"]),
                          _lib.i32ptr(k["mono_pt"]), _lib.i32ptr(k["mono_kf"]), _lib.dptr(k["mono_obs"]),
                          _lib.dptr(k["mono_info"]), _lib.i32ptr(k["st_pt"]), _lib.i32ptr(k["st_kf"]),
                          _lib.dptr(k["st_obs"]), _lib.dptr(k["st_info"]), _lib.i32ptr(k["oe_kf"]),
                          _lib.i32ptr(k["oe_obj"]), _lib.dptr(k["oe_meas"]), float(s["oe_info"]))
        h = C.c_void_p()
        _lib.check(L.qsp_ba_create(C.byref(sc), int(device), C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().qsp_ba_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_shard(self, rank, world, allreduce):
        """landmark sharding over `world` ranks; `allreduce(dev_ptr: int, count: int, hip_stream: int)` sums `count` float64
        at the device address in place over all ranks (qsp_slam_amd.parallel.TorchAllreduce wraps torch.distributed)."""
        def _cb(ctx, buf, n, stream):
            try:
                allreduce(int(buf), int(n), int(stream or 0))
                return 0
            except Exception as e:          # never let an exception cross the C boundary
                print("qsp all-reduce callback failed:", repr(e))
                return 1
        self._cb = _lib.ALLREDUCE_FN(_cb) if world > 1 else _lib.ALLREDUCE_FN(0)
        _lib.check(_lib.lib().qsp_ba_set_shard(self.handle, int(rank), int(world), self._cb, None))

    def set_shard_rccl(self, comm):
        """landmark sharding with the collectives issued by the library: ncclAllReduce on the problem's own stream
        (qsp_ba_set_shard_rccl).  `comm` is a qsp_slam_amd.parallel.RcclComm (one rank per GPU)."""
        self._comm = comm                       # keep the communicator alive as long as the problem uses it
        _lib.check(_lib.lib().qsp_ba_set_shard_rccl(self.handle, int(comm.rank), int(comm.world), comm.nccl()))

    def set_object_elimination(self, on=True):
        """objects eliminated in closed form in front of the dense solve (default) or kept inside it (qsp_ba_set_option)"""
        _lib.check(_lib.lib().qsp_ba_set_option(self.handle, 1, 1 if on else 0))

    def set_cholesky_chain(self, on=True):
        """the dense factorisation as one launch (a resident chain workgroup + tile workgroups taking tickets; the default) or as
        one launch per block step; same bits either way (QSP_BA_OPT_CHOLESKY_CHAIN)"""
        _lib.check(_lib.lib().qsp_ba_set_option(self.handle, 2, 1 if on else 0))

    @property
    def cholesky_chain(self):
        prof = _lib.BaProfile()
        L = _lib.lib()
        # (qsp_ba_profile reports and sets the profiling switch: read it, then put the switch back)
        _lib.check(L.qsp_ba_profile(self.handle, 1 if getattr(self, "_profiling", False) else 0, C.byref(prof)))
        return bool(prof.cholesky_chain)

    @property
    def schur_form(self):
        """how the last trial of the last solve built the reduced camera system: 0 key-frame pair lists, 1 per landmark (FP64
        atomics), 2 block rows (LDS atomics), -1 none was built (qsp_ba_stats.schur_form)"""
        prof = _lib.BaProfile()
        _lib.check(_lib.lib().qsp_ba_profile(self.handle, 1 if getattr(self, "_profiling", False) else 0, C.byref(prof)))
        return int(prof.schur_form)

    def set_deterministic(self, on=True):
        """no atomics in the Schur complement: repeated runs give the same bits (qsp_ba_set_deterministic)"""
        _lib.check(_lib.lib().qsp_ba_set_deterministic(self.handle, 1 if on else 0))

    def set_levels(self, mono=None, stereo=None, obj=None):
        def p(a):
            return _lib.c_uint8_p() if a is None else _lib.u8ptr(_arr(a, np.uint8))
        keep = [None if a is None else _arr(a, np.uint8) for a in (mono, stereo, obj)]
        _lib.check(_lib.lib().qsp_ba_set_levels(self.handle, *[(_lib.c_uint8_p() if a is None else _lib.u8ptr(a))
                                                               for a in keep]))

    def optimize(self, n_iter, delta_mono=0.0, delta_stereo=0.0, delta_obj=0.0, stop=None):
        tr = Trace(n_iter)
        flag = _lib.c_uint8_p() if stop is None else _lib.u8ptr(stop)
        _lib.check(_lib.lib().qsp_ba_optimize(self.handle, int(n_iter), float(delta_mono), float(delta_stereo),
                                              float(delta_obj), flag, C.byref(tr.c)))
        d = tr.dict()
        kh, oh, ph = self.index()
        d.update(kf_hidx=kh, obj_hidx=oh, pt_hidx=ph)
        return d

    def local_joint_ba(self, stop=None):
        t1, t2 = Trace(5), Trace(10)
        flag = _lib.c_uint8_p() if stop is None else _lib.u8ptr(stop)
        _lib.check(_lib.lib().qsp_ba_local_joint(self.handle, flag, C.byref(t1.c), C.byref(t2.c)))
        return t1.dict(), t2.dict()

    def index(self):
        kh = np.zeros(max(self.n_kf, 1), np.int32)
        oh = np.zeros(max(self.n_obj, 1), np.int32)
        ph = np.zeros(max(self.n_pt, 1), np.int32)
        _lib.check(_lib.lib().qsp_ba_get_index(self.handle, _lib.i32ptr(kh), _lib.i32ptr(oh), _lib.i32ptr(ph)))
        return kh[: self.n_kf], oh[: self.n_obj], ph[: self.n_pt]

    def state(self):
        kf = np.zeros((max(self.n_kf, 1), 7))
        pt = np.zeros((max(self.n_pt, 1), 3))
        ob = np.zeros((max(self.n_obj, 1), 7))
        _lib.check(_lib.lib().qsp_ba_get_state(self.handle, _lib.dptr(kf), _lib.dptr(pt), _lib.dptr(ob)))
        return kf[: self.n_kf], pt[: self.n_pt], ob[: self.n_obj]

    def set_state(self, kf=None, pt=None, ob=None):
        keep = [None if a is None else _arr(a, np.float64) for a in (kf, pt, ob)]
        _lib.check(_lib.lib().qsp_ba_set_state(self.handle, *[(_lib.c_double_p() if a is None else _lib.dptr(a))
                                                              for a in keep]))

    def edges(self):
        cm, cs, co = np.zeros(max(self.nm, 1)), np.zeros(max(self.ns, 1)), np.zeros(max(self.no, 1))
        pm, ps = np.zeros(max(self.nm, 1), np.uint8), np.zeros(max(self.ns, 1), np.uint8)
        _lib.check(_lib.lib().qsp_ba_get_edges(self.handle, _lib.dptr(cm), _lib.dptr(cs), _lib.dptr(co), _lib.u8ptr(pm),
                                               _lib.u8ptr(ps)))
        return dict(mono_chi2=cm[: self.nm], st_chi2=cs[: self.ns], oe_chi2=co[: self.no],
                    mono_pos=pm[: self.nm].astype(bool), st_pos=ps[: self.ns].astype(bool))

    def profile(self, enable=True):
        self._profiling = bool(enable)
        p = _lib.BaProfile()
        _lib.check(_lib.lib().qsp_ba_profile(self.handle, 1 if enable else 0, C.byref(p)))
        return p


def release_caches():
    """give back the streams, device chunks and pinned buffers qsp_ba_destroy keeps for the next problem (qsp_ba_release_caches)"""
    _lib.lib().qsp_ba_release_caches()


class PoseOptimizer(object):
    """Optimizer::PoseOptimization (reference src/Optimizer.cc:244-456) on flattened inputs, one kernel launch per call
    (qsp_pose_optimize, include/qsp_hip.h)."""

    def __init__(self, max_points=4096, device=0):
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().qsp_pose_optimizer_create(int(device), int(max_points), C.byref(self.handle)))

    def close(self):
        if self.handle is not None and self.handle.value:
            _lib.lib().qsp_pose_optimizer_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize(self, K, pose, X, obs, info, stereo):
        """K (5,) fx fy cx cy bf; pose (7,) T_cw; X (n,3); obs (n,3) u v u_right; info (n,); stereo (n,) 0/1.
        Returns dict(pose (7,), outlier (n,) uint8, n_inliers, iters (4,), trace (4,10,3) chi2 / lambda / trials)."""
        n = int(np.size(info))                 # (_arr pads empty arrays so that their pointers stay valid)
        info = _arr(info, np.float64)
        K, pose = _arr(K, np.float64), _arr(pose, np.float64)
        X, obs = _arr(np.reshape(X, (-1, 3)), np.float64), _arr(np.reshape(obs, (-1, 3)), np.float64)
        stereo = _arr(stereo, np.uint8)
        out = np.zeros(7)
        outlier = np.zeros(max(n, 1), np.uint8)
        ninl = C.c_int32()
        tr = _lib.PoseTrace()
        _lib.check(_lib.lib().qsp_pose_optimize(self.handle, n, _lib.dptr(K), _lib.dptr(pose), _lib.dptr(X), _lib.dptr(obs),
                                                _lib.dptr(info), _lib.u8ptr(stereo), _lib.dptr(out), _lib.u8ptr(outlier),
                                                C.byref(ninl), C.byref(tr)))
        trace = np.array(tr.trace[:], np.float64).reshape(4, 10, 3)
        return dict(pose=out, outlier=outlier[:n], n_inliers=int(ninl.value), iters=np.array(tr.iters[:], np.int32), trace=trace)


def optimize_sim3_batch(candidates, th2, fix_scale, device=0, trace=False):
    """Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1050-1245) for every loop candidate in ONE kernel launch
    (qsp_sim3_optimize_batch, include/qsp_hip.h).  `candidates`: list of dicts with K1, K2 (4,) fx fy cx cy; sim3 (8,) tx ty tz
    qx qy qz qw s of S12; P1c, P2c (n,3) the matched points in their own camera frames; obs1, obs2 (n,2); info1, info2 (n,).
    Returns one dict per candidate: sim3 (8,), inlier (n,) uint8, n_inliers and, with trace=True, iters (2,) and trace (2,10,3)
    chi2 / lambda / trials of the two optimize calls."""
    nc = len(candidates)
    if nc == 0:
        return []
    f64 = lambda key, w: [np.asarray(c[key], np.float64).reshape(-1, w) for c in candidates]
    P1, P2, o1, o2 = f64("P1c", 3), f64("P2c", 3), f64("obs1", 2), f64("obs2", 2)
    i1, i2 = f64("info1", 1), f64("info2", 1)
    counts = [len(a) for a in P1]
    for arrs in (P2, o1, o2, i1, i2):
        if [len(a) for a in arrs] != counts:
            raise ValueError("optimize_sim3_batch: the match arrays of a candidate differ in length")
    off = np.zeros(nc + 1, np.int32)
    off[1:] = np.cumsum(counts)
    nm = int(off[-1])
    cat = lambda arrs: _arr(np.concatenate(arrs), np.float64)
    P1, P2, o1, o2, i1, i2 = cat(P1), cat(P2), cat(o1), cat(o2), cat(i1), cat(i2)
    K1 = _arr(np.stack([np.asarray(c["K1"], np.float64).reshape(4) for c in candidates]), np.float64)
    K2 = _arr(np.stack([np.asarray(c["K2"], np.float64).reshape(4) for c in candidates]), np.float64)
    S0 = _arr(np.stack([np.asarray(c["sim3"], np.float64).reshape(8) for c in candidates]), np.float64)
    out = np.zeros((nc, 8))
    inlier = np.zeros(max(nm, 1), np.uint8)
    ninl = np.zeros(nc, np.int32)
    tr = (_lib.Sim3Trace * nc)() if trace else None
    _lib.check(_lib.lib().qsp_sim3_optimize_batch(int(device), nc, _lib.i32ptr(off), _lib.dptr(K1), _lib.dptr(K2), _lib.dptr(S0),
                                                  _lib.dptr(P1), _lib.dptr(P2), _lib.dptr(o1), _lib.dptr(o2), _lib.dptr(i1),
                                                  _lib.dptr(i2), float(th2), 1 if fix_scale else 0, _lib.dptr(out),
                                                  _lib.u8ptr(inlier), _lib.i32ptr(ninl), tr))
    res = []
    for c in range(nc):
        r = dict(sim3=out[c].copy(), inlier=inlier[off[c]:off[c + 1]].copy(), n_inliers=int(ninl[c]))
        if trace:
            r["iters"] = np.array(tr[c].iters[:], np.int32)
            r["trace"] = np.array(tr[c].trace[:], np.float64).reshape(2, 10, 3)
        res.append(r)
    return res


def optimize_sim3(candidate, th2, fix_scale, device=0, trace=False):
    """the batch of one"""
    return optimize_sim3_batch([candidate], th2, fix_scale, device=device, trace=trace)[0]


def sim3_ransac_iterations(n, prob=0.99, min_inliers=20, max_its=300):
    """Sim3Solver::SetRansacParameters (reference src/Sim3Solver.cc:114-138): the iterations a candidate of n kept matches runs,
    with the reference's float epsilon.  0 below min_inliers matches: iterate() returns nothing there (:146-150)."""
    n = int(n)
    if n < min_inliers:
        return 0
    if n == min_inliers:
        its = 1
    else:
        eps = float(np.float32(min_inliers) / np.float32(n))                       # float epsilon = (float)mRansacMinInliers/N
        its = int(np.ceil(np.log(1.0 - prob) / np.log(1.0 - eps ** 3)))
    return max(1, min(its, int(max_its)))


def draw_triples(n, its, rng):
    """The minimal sets of `its` iterations over n matches, drawn as iterate() draws them (:163-177: an index of the available
    list, which then takes the list's last entry and shrinks), from a numpy Generator.  (its,3) int32, three different indices."""
    out = np.zeros((int(its), 3), np.int32)
    for h in range(int(its)):
        avail = list(range(int(n)))
        for i in range(3):
            r = int(rng.integers(0, len(avail)))                                   # RandomInt(0, size - 1)
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def sim3_ransac_batch(cands, min_inliers=20, fix_scale=False, counts=False, device=0):
    """Sim3Solver (reference src/Sim3Solver.cc) for every loop candidate in ONE call (qsp_sim3_ransac_batch, include/qsp_hip.h).
    `cands`: list of dicts with K1, K2 (4,) fx fy cx cy; X1c, X2c (n,3) the matched points in their own camera frames; sigma2_1,
    sigma2_2 (n,) mvLevelSigma2 of the key points' octaves; triples (k,3) the minimal sets (draw_triples); n_its, the iterations
    to run (default k; sim3_ransac_iterations).  Returns one dict per candidate: first_it (1-based, 0 = no hypothesis had more
    than min_inliers inliers), R (3,3), t (3,), s, inlier (n,) uint8, n_inliers and, with counts=True, hyp_inliers (k,), the count
    of every hypothesis."""
    nc = len(cands)
    if nc == 0:
        return []
    f32 = lambda key, w: [np.asarray(c[key], np.float32).reshape(-1, w) for c in cands]
    X1, X2, s1, s2 = f32("X1c", 3), f32("X2c", 3), f32("sigma2_1", 1), f32("sigma2_2", 1)
    n = [len(a) for a in X1]
    for arrs in (X2, s1, s2):
        if [len(a) for a in arrs] != n:
            raise ValueError("sim3_ransac_batch: the match arrays of a candidate differ in length")
    tri = [np.asarray(c["triples"], np.int32).reshape(-1, 3) for c in cands]
    its = np.array([int(c.get("n_its", len(t))) for c, t in zip(cands, tri)], np.int32)
    off, toff = np.zeros(nc + 1, np.int32), np.zeros(nc + 1, np.int32)
    off[1:], toff[1:] = np.cumsum(n), np.cumsum([len(t) for t in tri])
    nm, nt = int(off[-1]), int(toff[-1])
    cat = lambda arrs, dt: _arr(np.concatenate(arrs), dt)
    X1, X2, s1, s2, tri = cat(X1, np.float32), cat(X2, np.float32), cat(s1, np.float32), cat(s2, np.float32), cat(tri, np.int32)
    K1 = _arr(np.stack([np.asarray(c["K1"], np.float32).reshape(4) for c in cands]), np.float32)
    K2 = _arr(np.stack([np.asarray(c["K2"], np.float32).reshape(4) for c in cands]), np.float32)
    first, ninl = np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    R, t, s = np.zeros((nc, 9), np.float32), np.zeros((nc, 3), np.float32), np.zeros(nc, np.float32)
    inlier = np.zeros(max(nm, 1), np.uint8)
    hyp = np.zeros(max(nt, 1), np.int32) if counts else None
    _lib.check(_lib.lib().qsp_sim3_ransac_batch(int(device), nc, _lib.i32ptr(off), _lib.i32ptr(its), _lib.i32ptr(toff), _lib.i32ptr(tri),
                                                _lib.fptr(K1), _lib.fptr(K2), _lib.fptr(X1), _lib.fptr(X2), _lib.fptr(s1), _lib.fptr(s2),
                                                int(min_inliers), 1 if fix_scale else 0, _lib.i32ptr(first), _lib.fptr(R), _lib.fptr(t),
                                                _lib.fptr(s), _lib.u8ptr(inlier), _lib.i32ptr(ninl),
                                                _lib.i32ptr(hyp) if counts else None))
    res = []
    for c in range(nc):
        r = dict(first_it=int(first[c]), R=R[c].reshape(3, 3).copy(), t=t[c].copy(), s=np.float32(s[c]),
                 inlier=inlier[off[c]:off[c + 1]].copy(), n_inliers=int(ninl[c]))
        if counts:
            r["hyp_inliers"] = hyp[toff[c]:toff[c + 1]].copy()
        res.append(r)
    return res


def _orb_frame(f, keep):
    """qsp_orb_frame over the arrays of a frame dict (search_by_sim3_batch); `keep` holds what the pointers point into"""
    n = int(np.size(f["octave"]))
    a = dict(kp=_arr(np.reshape(f["kp"], (-1, 2)), np.float32), octave=_arr(np.reshape(f["octave"], -1), np.int32),
             desc=_arr(np.reshape(f["desc"], (-1, 32)), np.uint8), sf=_arr(np.reshape(f["scale_factors"], -1), np.float32),
             has_point=_arr(np.reshape(f["has_point"], -1), np.uint8), Xw=_arr(np.reshape(f["Xw"], (-1, 3)), np.float32),
             dist_min_inv=_arr(np.reshape(f["dist_min_inv"], -1), np.float32), dist_max_inv=_arr(np.reshape(f["dist_max_inv"], -1), np.float32),
             dist_max=_arr(np.reshape(f["dist_max"], -1), np.float32), mp_desc=_arr(np.reshape(f["mp_desc"], (-1, 32)), np.uint8))
    for key, w in (("kp", 2), ("desc", 32), ("has_point", 1), ("Xw", 3), ("dist_min_inv", 1), ("dist_max_inv", 1), ("dist_max", 1),
                   ("mp_desc", 32)):
        if int(np.size(f[key])) != w * n:
            raise ValueError("search_by_sim3_batch: %s does not hold %d values per key point" % (key, w))
    keep.append(a)
    o = _lib.OrbFrame()
    o.n = n
    o.kp, o.octave, o.desc = _lib.fptr(a["kp"]), _lib.i32ptr(a["octave"]), _lib.u8ptr(a["desc"])
    o.min_x, o.max_x, o.min_y, o.max_y = [float(v) for v in f["bounds"]]
    o.grid_cols, o.grid_rows = int(f["grid"][0]), int(f["grid"][1])
    o.grid_w_inv, o.grid_h_inv = float(f["grid"][2]), float(f["grid"][3])
    o.n_levels, o.log_scale, o.scale_factors = int(np.size(f["scale_factors"])), float(f["log_scale"]), _lib.fptr(a["sf"])
    o.Rcw[:] = [float(v) for v in np.reshape(f["Rcw"], 9)]
    o.tcw[:] = [float(v) for v in np.reshape(f["tcw"], 3)]
    o.has_point, o.Xw, o.mp_desc = _lib.u8ptr(a["has_point"]), _lib.fptr(a["Xw"]), _lib.u8ptr(a["mp_desc"])
    o.dist_min_inv, o.dist_max_inv, o.dist_max = _lib.fptr(a["dist_min_inv"]), _lib.fptr(a["dist_max_inv"]), _lib.fptr(a["dist_max"])
    return o


def search_by_sim3_batch(kf1, cands, tap=False, device=0):
    """ORBmatcher::SearchBySim3 (reference src/ORBmatcher.cc:1102-1326) for every loop candidate in ONE call
    (qsp_search_by_sim3_batch, include/qsp_hip.h).  A frame is a dict: kp (n,2), octave (n,), desc (n,32) uint8, bounds (min_x,
    max_x, min_y, max_y), grid (cols, rows, width_inv, height_inv), log_scale, scale_factors (n_levels,), Rcw (3,3), tcw (3,) and
    per slot has_point (n,), Xw (n,3), dist_min_inv, dist_max_inv, dist_max (n,), mp_desc (n,32) uint8.  `kf1` is the current key
    frame; `cands`: list of dicts with kf2 (a frame), K (4,) fx fy cx cy of key frame 1, s12, R12 (3,3), t12 (3,), th (default 7.5),
    pre1 (n1,), pre2 (n2,) (default: none set).  Returns one dict per candidate: match12 (n1,) int32 (-1 = none), n_found and,
    with tap=True, best1, dist1 (n1,), best2, dist2 (n2,): the two passes before the agreement step."""
    nc = len(cands)
    if nc == 0:
        return []
    keep = []
    f1 = _orb_frame(kf1, keep)
    n1 = int(f1.n)
    f2 = (_lib.OrbFrame * nc)(*[_orb_frame(c["kf2"], keep) for c in cands])
    n2 = [int(f.n) for f in f2]
    off2 = np.zeros(nc + 1, np.int32)
    off2[1:] = np.cumsum(n2)
    nm2 = int(off2[-1])
    u8 = lambda c, key, n: (np.zeros(n, np.uint8) if c.get(key) is None else np.asarray(c[key]).astype(bool).astype(np.uint8).reshape(-1))
    pre1, pre2 = [u8(c, "pre1", n1) for c in cands], [u8(c, "pre2", n) for c, n in zip(cands, n2)]
    if [len(p) for p in pre1] != [n1] * nc or [len(p) for p in pre2] != n2:
        raise ValueError("search_by_sim3_batch: pre1 / pre2 do not match the key-point counts")
    pre1, pre2 = _arr(np.concatenate(pre1), np.uint8), _arr(np.concatenate(pre2), np.uint8)
    K = _arr(np.stack([np.asarray(c["K"], np.float32).reshape(4) for c in cands]), np.float32)
    s12 = _arr([c["s12"] for c in cands], np.float32)
    R12 = _arr(np.stack([np.asarray(c["R12"], np.float32).reshape(9) for c in cands]), np.float32)
    t12 = _arr(np.stack([np.asarray(c["t12"], np.float32).reshape(3) for c in cands]), np.float32)
    th = _arr([c.get("th", 7.5) for c in cands], np.float32)
    i = _lib.SearchSim3In(nc, C.pointer(f1), f2, _lib.i32ptr(off2), _lib.fptr(K), _lib.fptr(s12), _lib.fptr(R12), _lib.fptr(t12),
                          _lib.fptr(th), _lib.u8ptr(pre1), _lib.u8ptr(pre2))
    match, found = np.zeros(max(nc * n1, 1), np.int32), np.zeros(nc, np.int32)
    b1, d1, b2, d2 = (np.zeros(max(n, 1), np.int32) for n in (nc * n1, nc * n1, nm2, nm2))
    o = _lib.SearchSim3Out(_lib.i32ptr(match), _lib.i32ptr(found), *([_lib.i32ptr(a) for a in (b1, d1, b2, d2)] if tap else [None] * 4))
    _lib.check(_lib.lib().qsp_search_by_sim3_batch(int(device), C.byref(i), C.byref(o)))
    res = []
    for c in range(nc):
        r = dict(match12=match[c * n1:(c + 1) * n1].copy(), n_found=int(found[c]))
        if tap:
            r.update(best1=b1[c * n1:(c + 1) * n1].copy(), dist1=d1[c * n1:(c + 1) * n1].copy(),
                     best2=b2[off2[c]:off2[c + 1]].copy(), dist2=d2[off2[c]:off2[c + 1]].copy())
        res.append(r)
    return res


def _bow_frame(f, keep):
    """qsp_bow_frame over the arrays of a frame dict (search_by_bow_batch); `keep` holds what the pointers point into"""
    n = int(np.size(f["angle"]))
    a = dict(desc=_arr(np.reshape(f["desc"], (-1, 32)), np.uint8), angle=_arr(np.reshape(f["angle"], -1), np.float32),
             node_id=_arr(np.reshape(f["node_id"], -1), np.int32), node_off=_arr(np.reshape(f["node_off"], -1), np.int32),
             feat=_arr(np.reshape(f["feat"], -1), np.int32))
    if int(np.size(f["desc"])) != 32 * n:
        raise ValueError("search_by_bow_batch: desc does not hold 32 bytes per key point")
    nn = int(np.size(f["node_id"]))
    if int(np.size(f["node_off"])) != nn + 1:
        raise ValueError("search_by_bow_batch: node_off holds one entry more than node_id")
    if int(np.size(f["feat"])) < int(a["node_off"][nn]):
        raise ValueError("search_by_bow_batch: feat is shorter than node_off says")
    o = _lib.BowFrame()
    o.n, o.n_nodes = n, nn
    o.desc, o.angle = _lib.u8ptr(a["desc"]), _lib.fptr(a["angle"])
    if f.get("eligible") is not None:
        a["eligible"] = _arr(np.asarray(f["eligible"]).astype(bool).reshape(-1), np.uint8)
        if int(np.size(f["eligible"])) != n:
            raise ValueError("search_by_bow_batch: eligible does not hold one value per key point")
        o.eligible = _lib.u8ptr(a["eligible"])
    o.node_id, o.node_off, o.feat = _lib.i32ptr(a["node_id"]), _lib.i32ptr(a["node_off"]), _lib.i32ptr(a["feat"])
    keep.append(a)
    return o


def search_by_bow_batch(shared, cands, *, shared_is_source=True, th=50, th_inclusive=False, nn_ratio=0.75, check_orientation=True,
                        tap=False, device=0):
    """ORBmatcher::SearchByBoW for every candidate in ONE call (qsp_search_by_bow_batch, include/qsp_hip.h).  A frame is a dict:
    desc (n,32) uint8, angle (n,), eligible (n,) or None (= every slot), and its feature vector in CSR form: node_id (ascending),
    node_off, feat (the indices of each node in the reference's order).  shared_is_source=True is the key-frame overload of loop
    closing (reference src/ORBmatcher.cc:522-655): `shared` is key frame 1, the source of every candidate.  False is the frame
    overload of relocalisation (:159-288, there with th_inclusive=True): every candidate is the source, `shared` the target.
    Returns one dict per candidate: match (source slots,) int32 target index or -1, n_matches and, with tap=True, match_raw (before
    the rotation cull), dist, hist (30,), ind (3,)."""
    nc = len(cands)
    if nc == 0:
        return []
    keep = []
    f0 = _bow_frame(shared, keep)
    fc = (_lib.BowFrame * nc)(*[_bow_frame(c, keep) for c in cands])
    n0, n = int(f0.n), [int(f.n) for f in fc]
    off = np.zeros(nc + 1, np.int64)
    off[1:] = np.cumsum(n) if not shared_is_source else n0 * np.arange(1, nc + 1)
    i = _lib.SearchBowIn(nc, 1 if shared_is_source else 0, C.pointer(f0), fc, int(th), 1 if th_inclusive else 0, float(nn_ratio),
                         1 if check_orientation else 0)
    n_out = max(int(off[-1]), 1)
    match, count = np.zeros(n_out, np.int32), np.zeros(nc, np.int32)
    raw, dist, hist, ind = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((nc, 30), np.int32), np.zeros((nc, 3), np.int32)
    o = _lib.SearchBowOut(_lib.i32ptr(match), _lib.i32ptr(count), *([_lib.i32ptr(a) for a in (raw, dist, hist, ind)] if tap else [None] * 4))
    _lib.check(_lib.lib().qsp_search_by_bow_batch(int(device), C.byref(i), C.byref(o)))
    res = []
    for c in range(nc):
        r = dict(match=match[off[c]:off[c + 1]].copy(), n_matches=int(count[c]))
        if tap:
            r.update(match_raw=raw[off[c]:off[c + 1]].copy(), dist=dist[off[c]:off[c + 1]].copy(), hist=hist[c].copy(), ind=ind[c].copy())
        res.append(r)
    return res


def _tri_frame(f, keep, target):
    """qsp_tri_frame over the arrays of a frame dict (search_for_triangulation_batch): the qsp_bow_frame and the arrays beside it"""
    o = _lib.TriFrame()
    o.bow = _bow_frame(f, keep)
    n = int(o.bow.n)
    a = dict(xy=_arr(np.reshape(f["xy"], (-1, 2)), np.float32), stereo=_arr(np.asarray(f["stereo"]).astype(bool).reshape(-1), np.uint8))
    widths = dict(xy=2, stereo=1)
    if target:
        a.update(sigma2=_arr(np.reshape(f["sigma2"], -1), np.float32), scale=_arr(np.reshape(f["scale"], -1), np.float32))
        widths.update(sigma2=1, scale=1)
        o.sigma2, o.scale = _lib.fptr(a["sigma2"]), _lib.fptr(a["scale"])
    for key, w in widths.items():
        if int(np.size(f[key])) != w * n:
            raise ValueError("search_for_triangulation_batch: %s does not hold %d values per key point" % (key, w))
    o.xy, o.stereo = _lib.fptr(a["xy"]), _lib.u8ptr(a["stereo"])
    keep.append(a)
    return o


def search_for_triangulation_batch(shared, cands, F12, exy, th=50, only_stereo=False, check_orientation=False, tap=False, device=0):
    """ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:657-823) for every covisible neighbour in ONE call
    (qsp_search_for_triangulation_batch, include/qsp_hip.h).  A frame is the dict of search_by_bow_batch -- desc (n,32) uint8, angle
    (n,), eligible (n,) (1 = the slot holds no map point; None = every slot), node_id, node_off, feat -- with xy (n,2) and stereo
    (n,) beside it and, for the neighbours, sigma2 (n,) and scale (n,) gathered through the key point's octave.  `shared` is the
    current key frame, the source of every neighbour in `cands`; F12 (n_cand,3,3) and exy (n_cand,2) are each neighbour's
    fundamental matrix and epipole.  Returns one dict per neighbour: match (shared n,) int32 target index or -1, n_matches and, with
    tap=True, match_raw (before the rotation cull), dist, hist (30,), ind (3,)."""
    nc = len(cands)
    if nc == 0:
        return []
    keep = []
    f1 = _tri_frame(shared, keep, False)
    f2 = (_lib.TriFrame * nc)(*[_tri_frame(c, keep, True) for c in cands])
    F = _arr(np.reshape(F12, (-1, 9)), np.float32)
    e = _arr(np.reshape(exy, (-1, 2)), np.float32)
    if len(F) != nc or len(e) != nc:
        raise ValueError("search_for_triangulation_batch: F12 and exy hold one entry per neighbour")
    n1 = int(f1.bow.n)
    i = _lib.SearchTriIn(nc, C.pointer(f1), f2, _lib.fptr(F), _lib.fptr(e), int(th), 1 if only_stereo else 0, 1 if check_orientation else 0)
    n_out = max(nc * n1, 1)
    match, count = np.zeros(n_out, np.int32), np.zeros(nc, np.int32)
    raw, dist, hist, ind = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((nc, 30), np.int32), np.zeros((nc, 3), np.int32)
    o = _lib.SearchTriOut(_lib.i32ptr(match), _lib.i32ptr(count), *([_lib.i32ptr(a) for a in (raw, dist, hist, ind)] if tap else [None] * 4))
    _lib.check(_lib.lib().qsp_search_for_triangulation_batch(int(device), C.byref(i), C.byref(o)))
    res = []
    for c in range(nc):
        r = dict(match=match[c * n1:(c + 1) * n1].copy(), n_matches=int(count[c]))
        if tap:
            r.update(match_raw=raw[c * n1:(c + 1) * n1].copy(), dist=dist[c * n1:(c + 1) * n1].copy(), hist=hist[c].copy(), ind=ind[c].copy())
        res.append(r)
    return res


def _fuse_target(f, keep):
    """qsp_orb_frame over what qsp_fuse_batch reads of a target dict (the map-point fields stay NULL)"""
    n = int(np.size(f["octave"]))
    a = dict(kp=_arr(np.reshape(f["kp"], (-1, 2)), np.float32), octave=_arr(np.reshape(f["octave"], -1), np.int32),
             desc=_arr(np.reshape(f["desc"], (-1, 32)), np.uint8), sf=_arr(np.reshape(f["scale_factors"], -1), np.float32))
    for key, w in (("kp", 2), ("desc", 32), ("u_right", 1)):
        if int(np.size(f[key])) != w * n:
            raise ValueError("fuse_batch: %s does not hold %d values per key point" % (key, w))
    keep.append(a)
    o = _lib.OrbFrame()
    o.n = n
    o.kp, o.octave, o.desc = _lib.fptr(a["kp"]), _lib.i32ptr(a["octave"]), _lib.u8ptr(a["desc"])
    o.min_x, o.max_x, o.min_y, o.max_y = [float(v) for v in f["bounds"]]
    o.grid_cols, o.grid_rows = int(f["grid"][0]), int(f["grid"][1])
    o.grid_w_inv, o.grid_h_inv = float(f["grid"][2]), float(f["grid"][3])
    o.n_levels, o.log_scale, o.scale_factors = int(np.size(f["scale_factors"])), float(f["log_scale"]), _lib.fptr(a["sf"])
    o.Rcw[:] = [float(v) for v in np.reshape(f["Rcw"], 9)]
    o.tcw[:] = [float(v) for v in np.reshape(f["tcw"], 3)]
    return o


def _fuse_in(targets, pool):
    """the qsp_fuse_in of fuse_batch, with `keep` (what its pointers point into, by name) and the pairs' offsets per target"""
    nt = len(targets)
    keep = []
    fr = (_lib.OrbFrame * nt)(*[_fuse_target(t, keep) for t in targets])
    a = dict(K=_arr(np.stack([np.asarray(t["K"], np.float32).reshape(5) for t in targets]), np.float32),
             Ow=_arr(np.stack([np.asarray(t["Ow"], np.float32).reshape(3) for t in targets]), np.float32),
             th=_arr([t["th"] for t in targets], np.float32),
             u_right_off=_arr(np.concatenate([[0], np.cumsum([fr[k].n for k in range(nt)])]), np.int32),
             u_right=_arr(np.concatenate([np.reshape(t["u_right"], -1) for t in targets] + [np.zeros(1)]), np.float32),
             inv_level_sigma2=np.zeros((nt, 16), np.float32),
             check_reprojection=_arr([1 if t["check"] else 0 for t in targets], np.uint8),
             Xw=_arr(np.reshape(pool["Xw"], (-1, 3)), np.float32), normal=_arr(np.reshape(pool["normal"], (-1, 3)), np.float32),
             dist_min_inv=_arr(np.reshape(pool["dist_min_inv"], -1), np.float32), dist_max_inv=_arr(np.reshape(pool["dist_max_inv"], -1), np.float32),
             dist_max=_arr(np.reshape(pool["dist_max"], -1), np.float32), desc=_arr(np.reshape(pool["desc"], (-1, 32)), np.uint8),
             list_off=_arr(np.concatenate([[0], np.cumsum([np.size(t["list"]) for t in targets])]), np.int64),
             list_idx=_arr(np.concatenate([np.reshape(t["list"], -1) for t in targets] + [np.zeros(1)]), np.int32))
    n_point = int(np.size(pool["dist_max"]))
    for key, w in (("Xw", 3), ("normal", 3), ("dist_min_inv", 1), ("dist_max_inv", 1), ("desc", 32)):
        if int(np.size(pool[key])) != w * n_point:
            raise ValueError("fuse_batch: the pool's %s does not hold %d values per point" % (key, w))
    for k, t in enumerate(targets):
        s = np.asarray(t["inv_level_sigma2"], np.float32).reshape(-1)
        if len(s) != fr[k].n_levels or len(s) > 16:
            raise ValueError("fuse_batch: inv_level_sigma2 holds one value per level, at most 16")
        a["inv_level_sigma2"][k, :len(s)] = s
    keep.append(a)
    i = _lib.FuseIn(nt, fr, _lib.fptr(a["K"]), _lib.fptr(a["Ow"]), _lib.fptr(a["th"]), _lib.i32ptr(a["u_right_off"]), _lib.fptr(a["u_right"]),
                    _lib.fptr(a["inv_level_sigma2"]), _lib.u8ptr(a["check_reprojection"]), n_point, _lib.fptr(a["Xw"]), _lib.fptr(a["normal"]),
                    _lib.fptr(a["dist_min_inv"]), _lib.fptr(a["dist_max_inv"]), _lib.fptr(a["dist_max"]), _lib.u8ptr(a["desc"]),
                    a["list_off"].ctypes.data_as(C.POINTER(C.c_int64)), _lib.i32ptr(a["list_idx"]))
    return i, keep, a["list_off"]


def fuse_batch(targets, pool, tap=False, device=0):
    """The match phase of both ORBmatcher::Fuse overloads (reference src/ORBmatcher.cc:825-975 and :977-1100) for every target key
    frame in ONE call (qsp_fuse_batch, include/qsp_hip.h).  `pool`: the map points all targets share, a dict of Xw (n,3), normal
    (n,3), dist_min_inv, dist_max_inv, dist_max (n,) and desc (n,32) uint8.  `targets`: list of dicts with kp (n,2), octave (n,),
    desc (n,32) uint8, bounds (min_x, max_x, min_y, max_y), grid (cols, rows, width_inv, height_inv), log_scale, scale_factors
    (n_levels,), Rcw (3,3), tcw (3,), K (5,) fx fy cx cy mbf, Ow (3,), th, u_right (n,), inv_level_sigma2 (n_levels,), check
    (True: the pose overload's reprojection test; False: the Sim3 overload) and list: the pool indices the target searches, in
    order.  Returns one dict per target: best_idx, best_dist (len(list),) int32 (-1 = none) and, with tap=True, reason and level."""
    nt = len(targets)
    if nt == 0:
        return []
    i, keep, off = _fuse_in(targets, pool)
    n_pair = int(off[-1])
    best, dist, why, lvl = (np.full(max(n_pair, 1), -1, np.int32) for _ in range(4))
    o = _lib.FuseOut(_lib.i32ptr(best), _lib.i32ptr(dist), *([_lib.i32ptr(why), _lib.i32ptr(lvl)] if tap else [None, None]))
    _lib.check(_lib.lib().qsp_fuse_batch(int(device), C.byref(i), C.byref(o)))
    res = []
    for k in range(nt):
        r = dict(best_idx=best[off[k]:off[k + 1]].copy(), best_dist=dist[off[k]:off[k + 1]].copy())
        if tap:
            r.update(reason=why[off[k]:off[k + 1]].copy(), level=lvl[off[k]:off[k + 1]].copy())
        res.append(r)
    return res


_PROJ_SRC = (("valid", "src_valid", np.uint8, 1), ("blocks", "src_blocks", np.uint8, 1), ("Xw", "Xw", np.float32, 3), ("desc", "desc", np.uint8, 32))
_PROJ_SRC_MODE = ((("normal", "normal", np.float32, 3), ("dist_min_inv", "dist_min_inv", np.float32, 1), ("dist_max_inv", "dist_max_inv", np.float32, 1),
                   ("dist_max", "dist_max", np.float32, 1)),
                  (("octave", "src_octave", np.int32, 1), ("angle", "src_angle", np.float32, 1)))
_PROJ_PTR = {np.uint8: _lib.u8ptr, np.float32: _lib.fptr, np.int32: _lib.i32ptr}
_PROJ_OUT = (("choice", np.int32), ("dist", np.int32), ("in_view", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32), ("proj_xr", np.float32),
             ("level", np.int32), ("view_cos", np.float32), ("reason", np.int32), ("dist2", np.int32), ("level_best", np.int32),
             ("level2", np.int32), ("bin", np.int32))            # per source; slot_src is per key point
_PROJ_TAPS = ("reason", "dist2", "level_best", "level2", "bin")
_PROJ_LOCAL = ("in_view", "proj_x", "proj_y", "proj_xr", "level", "view_cos", "dist2", "level_best", "level2")


def _proj_in(frame, sources, mode, th, nn_ratio, view_cos_limit, check_orientation, mono, last_Rcw, last_tcw):
    """the qsp_search_proj_in of search_by_projection and `keep`: what its pointers point into (the last entry by field name)"""
    mode = {"local": 0, "last": 1}.get(mode, mode)
    keep = []
    fr = _fuse_target(frame, keep)
    n = int(fr.n)
    ns = int(np.size(sources["valid"]))
    a = dict(u_right=_arr(np.append(np.reshape(frame["u_right"], -1), 0), np.float32),
             slot_blocked=_arr(np.append(np.reshape(frame["slot_blocked"], -1), 0) != 0, np.uint8),
             kp_angle=_arr(np.append(np.reshape(frame.get("kp_angle", np.zeros(n)), -1), 0), np.float32))
    for key in ("slot_blocked", "kp_angle"):
        if len(a[key]) != n + 1:
            raise ValueError("search_by_projection: %s does not hold one value per key point" % key)
    for key, field, dt, w in _PROJ_SRC + (_PROJ_SRC_MODE[mode] if mode in (0, 1) else ()):
        if key == "angle" and key not in sources:
            continue
        if int(np.size(sources[key])) != w * ns:
            raise ValueError("search_by_projection: the sources' %s does not hold %d values per source" % (key, w))
        a[field] = _arr(np.append(np.reshape(sources[key], -1), np.zeros(w)), dt)
    keep += [fr, a]
    i = _lib.SearchProjIn()
    i.mode, i.frame, i.n_src = int(mode), C.pointer(fr), ns
    i.K[:] = [float(v) for v in np.reshape(frame["K"], 5)]
    i.Ow[:] = [float(v) for v in np.reshape(frame.get("Ow", np.zeros(3)), 3)]
    i.mb = float(frame.get("mb", 0.0))
    i.th, i.nn_ratio, i.view_cos_limit = float(th), float(nn_ratio), float(view_cos_limit)
    i.check_orientation, i.mono = int(bool(check_orientation)), int(bool(mono))
    i.last_Rcw[:] = [float(v) for v in np.reshape(np.eye(3) if last_Rcw is None else last_Rcw, 9)]
    i.last_tcw[:] = [float(v) for v in np.reshape(np.zeros(3) if last_tcw is None else last_tcw, 3)]
    for field, arr in a.items():
        setattr(i, field, _PROJ_PTR[arr.dtype.type](arr))
    return i, keep


def search_by_projection(frame, sources, mode="local", th=1.0, nn_ratio=0.8, view_cos_limit=0.5, check_orientation=True, mono=False,
                         last_Rcw=None, last_tcw=None, tap=False, device=0):
    """Tracking's projection searches with the result of the reference's serial loop (qsp_search_by_projection, include/qsp_hip.h):
    mode "local" is Frame::isInFrustum + ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (reference
    src/ORBmatcher.cc:45-129), mode "last" is SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (:1328-1470).
    `frame`, the current frame: kp (n,2), octave (n,), desc (n,32) uint8, bounds, grid (cols, rows, width_inv, height_inv), log_scale,
    scale_factors, Rcw, tcw, K (5,) fx fy cx cy mbf, u_right (n,), slot_blocked (n,) and, by mode, Ow (3,) / mb and kp_angle (n,).
    `sources`, in the reference's loop order: valid, blocks (n_src,), Xw (n_src,3), desc (n_src,32) and, by mode, normal, dist_min_inv,
    dist_max_inv, dist_max / octave, angle.  Returns a dict: choice, dist (n_src,), slot_src (n,), n_matches, n_rounds; "local" adds
    in_view, proj_x, proj_y, proj_xr, level, view_cos; "last" adds hist (30,) and ind (3,); tap=True adds reason and, by mode, dist2,
    level_best, level2 / bin."""
    i, keep = _proj_in(frame, sources, mode, th, nn_ratio, view_cos_limit, check_orientation, mono, last_Rcw, last_tcw)
    local = i.mode == 0
    ns, n = int(i.n_src), int(keep[-2].n)
    o = _lib.SearchProjOut()
    res = dict(slot_src=np.full(n + 1, -1, np.int32))
    o.slot_src = _lib.i32ptr(res["slot_src"])
    o.ind[:] = [-1, -1, -1]
    for key, dt in _PROJ_OUT:
        if (key in _PROJ_TAPS and not tap) or (key in _PROJ_LOCAL and not local) or (key == "bin" and local):
            continue
        res[key] = np.zeros(ns + 1, dt) if dt != np.int32 or key == "level" else np.full(ns + 1, -1, np.int32)
        setattr(o, key, _PROJ_PTR[dt](res[key]))
    _lib.check(_lib.lib().qsp_search_by_projection(int(device), C.byref(i), C.byref(o)))
    res = {key: (v[:n] if key == "slot_src" else v[:ns]) for key, v in res.items()}
    res.update(n_matches=int(o.n_matches), n_rounds=int(o.n_rounds))
    if not local:
        res.update(hist=np.array(o.hist[:], np.int32), ind=np.array(o.ind[:], np.int32))
    return res


_PROJ_KF_SRC = (("valid", "src_valid", np.uint8, 1), ("Xw", "Xw", np.float32, 3), ("desc", "desc", np.uint8, 32),
                ("dist_min_inv", "dist_min_inv", np.float32, 1), ("dist_max_inv", "dist_max_inv", np.float32, 1),
                ("dist_max", "dist_max", np.float32, 1), ("normal", "normal", np.float32, 3), ("angle", "src_angle", np.float32, 1))
_PROJ_KF_OUT = (("choice", np.int32), ("dist", np.int32), ("reason", np.int32), ("level", np.int32), ("proj_x", np.float32),
                ("proj_y", np.float32), ("bin", np.int32))       # per source; slot_src is per key point


def decompose_scw(Scw):
    """(Rcw, tcw, Ow) of a 3x4 (or 4x4) float32 Sim3 `Scw` as ORBmatcher.cc:299-303 decomposes it with cv::Mat operations on CV_32F,
    the form OrbMatcherHip::FuseBatch and the Sim3 overload of OrbMatcherHip::SearchByProjection use: scw = (float)sqrt(row0 . row0)
    with the dot product summed in double, Rcw = sRcw / scw and tcw = t / scw as float32 products with (float)(1.0 / scw) (what
    cv::Mat's division by a scalar is), Ow = -Rcw^T tcw (rows summed in double, rounded once, negated).  Exact divisions where scw is
    a power of two."""
    f32, f64 = np.float32, np.float64
    S = np.asarray(Scw, f32)[:3, :4]
    r0 = S[0, :3].astype(f64)
    scw = f32(np.sqrt((r0[0] * r0[0] + r0[1] * r0[1]) + r0[2] * r0[2]))
    inv = f32(1.0 / f64(scw))
    R, t = (S[:, :3] * inv).astype(f32), (S[:, 3] * inv).astype(f32)
    Rt, t64 = R.T.astype(f64), t.astype(f64)
    Ow = -((Rt[:, 0] * t64[0] + Rt[:, 1] * t64[1]) + Rt[:, 2] * t64[2]).astype(f32)
    return R, t, Ow


def _proj_kf_in(frame, src, mode, th, orb_dist, check_orientation):
    """the qsp_search_proj_kf_in of search_by_projection_kf and `keep`: what its pointers point into (the last entry by field name)"""
    mode = {"reloc": 0, "sim3": 1}.get(mode, mode)
    keep = []
    n = int(np.size(frame["octave"]))
    fr = _fuse_target(dict(frame, u_right=np.zeros(n, np.float32)), keep)
    ns = int(np.size(src["valid"]))
    a = dict(slot_blocked=_arr(np.append(np.reshape(frame["slot_blocked"], -1), 0) != 0, np.uint8),
             kp_angle=_arr(np.append(np.reshape(frame.get("kp_angle", np.zeros(n)), -1), 0), np.float32))
    for key in ("slot_blocked", "kp_angle"):
        if len(a[key]) != n + 1:
            raise ValueError("search_by_projection_kf: %s does not hold one value per key point" % key)
    for key, field, dt, w in _PROJ_KF_SRC:
        if key in ("normal", "angle") and key not in src:
            continue
        if int(np.size(src[key])) != w * ns:
            raise ValueError("search_by_projection_kf: the sources' %s does not hold %d values per source" % (key, w))
        a[field] = _arr(np.append(np.reshape(src[key], -1), np.zeros(w)), dt)
    keep += [fr, a]
    i = _lib.SearchProjKfIn()
    i.mode, i.frame, i.n_src = int(mode), C.pointer(fr), ns
    i.K[:] = [float(v) for v in np.reshape(frame["K"], -1)[:4]]
    i.Ow[:] = [float(v) for v in np.reshape(frame["Ow"], 3)]
    i.th, i.orb_dist, i.check_orientation = float(th), int(orb_dist), int(bool(check_orientation))
    for field, arr in a.items():
        setattr(i, field, _PROJ_PTR[arr.dtype.type](arr))
    return i, keep


def search_by_projection_kf(frame, src, mode, th, orb_dist=50, check_orientation=False, device=0):
    """The relocalisation and Sim3 overloads of ORBmatcher::SearchByProjection with the result of the reference's serial loop
    (qsp_search_by_projection_kf, include/qsp_hip.h): mode "reloc" is SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const
    set<MapPoint*>& sAlreadyFound, th, ORBdist) (reference src/ORBmatcher.cc:1472-1599), mode "sim3" is SearchByProjection(KeyFrame*
    pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, th) (:290-403).
    `frame`, the frame searched: kp (n,2), octave (n,), desc (n,32) uint8, bounds, grid (cols, rows, width_inv, height_inv), log_scale,
    scale_factors, Rcw, tcw, Ow (for "sim3" the three of decompose_scw), K (at least 4,) fx fy cx cy, slot_blocked (n,) = the slot is
    non-null at entry and, with check_orientation, kp_angle (n,).  `src`, in the reference's loop order: valid (n_src,), Xw (n_src,3),
    desc (n_src,32), dist_min_inv, dist_max_inv, dist_max (n_src,) and normal (n_src,3) for "sim3" / angle (n_src,) for "reloc" with
    check_orientation.  Returns the same kind of dict as search_by_projection: choice, dist (n_src,), slot_src (n,), n_matches,
    n_rounds, hist (30,), ind (3,) and the taps reason, level, proj_x, proj_y, bin (n_src,)."""
    i, keep = _proj_kf_in(frame, src, mode, th, orb_dist, check_orientation)
    ns, n = int(i.n_src), int(keep[-2].n)
    o = _lib.SearchProjKfOut()
    res = dict(slot_src=np.full(n + 1, -1, np.int32))
    o.slot_src = _lib.i32ptr(res["slot_src"])
    o.ind[:] = [-1, -1, -1]
    for key, dt in _PROJ_KF_OUT:
        res[key] = np.zeros(ns + 1, dt) if dt != np.int32 or key == "level" else np.full(ns + 1, -1, np.int32)
        setattr(o, key, _PROJ_PTR[dt](res[key]))
    _lib.check(_lib.lib().qsp_search_by_projection_kf(int(device), C.byref(i), C.byref(o)))
    res = {key: (v[:n] if key == "slot_src" else v[:ns]) for key, v in res.items()}
    res.update(n_matches=int(o.n_matches), n_rounds=int(o.n_rounds), hist=np.array(o.hist[:], np.int32), ind=np.array(o.ind[:], np.int32))
    return res


_TRI_POSE = (("Rcw", 9), ("tcw", 3), ("Ow", 3))
_TRI_SCALARS = ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")
_TRI_ARRAYS = (("xy", "xy_un", 2), ("xy_raw", "xy", 2), ("u_right", "u_right", 1), ("depth", "depth", 1), ("sigma2", "sigma2", 1),
               ("scale", "scale", 1))           # (key of the frame dict, field of qsp_triangulate_frame, values per key point)
_TRI_TAPS = (("reason", np.int32, 1), ("path", np.int32, 1), ("cos_rays", np.float32, 1), ("z", np.float32, 2), ("err2", np.float32, 2),
             ("ratio_dist", np.float32, 1))


def _triangulate_frame(f, keep):
    """qsp_triangulate_frame over the geometry of a frame dict (triangulate_batch)"""
    o = _lib.TriangulateFrame()
    n = int(np.size(f["u_right"]))
    o.n = n
    for key, w in _TRI_POSE:
        getattr(o, key)[:] = [float(v) for v in np.asarray(f[key], np.float32).reshape(w)]
    for key in _TRI_SCALARS:
        setattr(o, key, float(np.float32(f[key])))
    a = {}
    for key, field, w in _TRI_ARRAYS:
        if int(np.size(f[key])) != w * n:
            raise ValueError("triangulate_batch: %s does not hold %d values per key point" % (key, w))
        a[key] = _arr(np.reshape(f[key], -1), np.float32)
        setattr(o, field, _lib.fptr(a[key]))
    keep.append(a)
    return o


def _triangulate_geom(kf1, kf2s, keep):
    nc = len(kf2s)
    f1 = _triangulate_frame(kf1, keep)
    f2 = (_lib.TriangulateFrame * nc)(*[_triangulate_frame(c, keep) for c in kf2s])
    keep += [f1, f2]
    return _lib.TriangulateGeom(nc, C.pointer(f1), f2, float(np.float32(kf1["ratio_factor"])))


def _triangulate_out(nc, n1, tap):
    """the qsp_triangulate_out of one call and the arrays behind it"""
    n = max(nc * n1, 1)
    a = dict(accept=np.zeros(n, np.uint8), first=np.zeros(n, np.uint8), x3D=np.zeros(3 * n, np.float32), n_new=np.zeros(max(nc, 1), np.int32))
    if tap:
        a.update({key: np.zeros(w * n, dt) for key, dt, w in _TRI_TAPS})
    o = _lib.TriangulateOut(_lib.u8ptr(a["accept"]), _lib.u8ptr(a["first"]), _lib.fptr(a["x3D"]), _lib.i32ptr(a["n_new"]))
    if tap:
        for key, dt, _ in _TRI_TAPS:
            setattr(o, key, _lib.i32ptr(a[key]) if dt is np.int32 else _lib.fptr(a[key]))
    return o, a


def _triangulate_results(a, nc, n1, tap):
    res = []
    for k in range(nc):
        s = slice(k * n1, (k + 1) * n1)
        r = dict(accept=a["accept"][s].astype(bool), first=a["first"][s].astype(bool), x3D=a["x3D"].reshape(-1, 3)[s].copy(), n_new=int(a["n_new"][k]))
        if tap:
            r.update({key: a[key].reshape((-1, w) if w > 1 else (-1,))[s].copy() for key, _, w in _TRI_TAPS})
        res.append(r)
    return res


def triangulate_batch(kf1, kf2s, match, tap=False, device=0):
    """The numeric part of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:467-607) for every covisible neighbour in
    ONE call (qsp_triangulate_batch, include/qsp_hip.h).  A frame is a dict of Rcw (3,3), tcw (3,), Ow (3,), fx fy cx cy invfx invfy
    mb mbf, and per key point xy (n,2) = mvKeysUn.pt (as in search_for_triangulation_batch), xy_raw (n,2) = mvKeys.pt, u_right, depth,
    sigma2 and scale (n,), the last two
    gathered through the octave; kf1 also holds ratio_factor = 1.5 * its mfScaleFactor.  `match` (n_cand, n1) int32 is the grid
    search_for_triangulation_batch returns: per slot of kf1 the neighbour's index or -1.  Returns one dict per neighbour: accept and
    first (n1,) bool -- first marks the points the reference would create --, x3D (n1,3), n_new and, with tap=True, reason, path,
    cos_rays, z (n1,2), err2 (n1,2), ratio_dist."""
    nc = len(kf2s)
    if nc == 0:
        return []
    keep = []
    g = _triangulate_geom(kf1, kf2s, keep)
    n1 = int(g.kf1[0].n)
    if int(np.size(match)) != nc * n1:
        raise ValueError("triangulate_batch: match holds one entry per neighbour and key point of kf1")
    m = _arr(np.reshape(match, -1), np.int32)
    o, a = _triangulate_out(nc, n1, tap)
    _lib.check(_lib.lib().qsp_triangulate_batch(int(device), C.byref(g), _lib.i32ptr(m), C.byref(o)))
    return _triangulate_results(a, nc, n1, tap)


def create_new_map_points_batch(shared, cands, F12, exy, th=50, only_stereo=False, check_orientation=False, tap=False, device=0):
    """search_for_triangulation_batch followed by triangulate_batch in ONE call (qsp_create_new_map_points_batch): one upload, four
    launches, one download; the match grid does not come back to the host in between.  Every frame dict holds what both calls
    read.  Returns one dict per neighbour with the keys of both."""
    nc = len(cands)
    if nc == 0:
        return []
    keep = []
    f1 = _tri_frame(shared, keep, False)
    f2 = (_lib.TriFrame * nc)(*[_tri_frame(c, keep, True) for c in cands])
    F = _arr(np.reshape(F12, (-1, 9)), np.float32)
    e = _arr(np.reshape(exy, (-1, 2)), np.float32)
    if len(F) != nc or len(e) != nc:
        raise ValueError("create_new_map_points_batch: F12 and exy hold one entry per neighbour")
    g = _triangulate_geom(shared, cands, keep)
    n1 = int(f1.bow.n)
    i = _lib.SearchTriIn(nc, C.pointer(f1), f2, _lib.fptr(F), _lib.fptr(e), int(th), 1 if only_stereo else 0, 1 if check_orientation else 0)
    n_out = max(nc * n1, 1)
    match, count = np.zeros(n_out, np.int32), np.zeros(nc, np.int32)
    raw, dist, hist, ind = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((nc, 30), np.int32), np.zeros((nc, 3), np.int32)
    so = _lib.SearchTriOut(_lib.i32ptr(match), _lib.i32ptr(count), *([_lib.i32ptr(a) for a in (raw, dist, hist, ind)] if tap else [None] * 4))
    o, a = _triangulate_out(nc, n1, tap)
    _lib.check(_lib.lib().qsp_create_new_map_points_batch(int(device), C.byref(i), C.byref(g), C.byref(so), C.byref(o)))
    res = _triangulate_results(a, nc, n1, tap)
    for c, r in enumerate(res):
        r.update(match=match[c * n1:(c + 1) * n1].copy(), n_matches=int(count[c]))
        if tap:
            r.update(match_raw=raw[c * n1:(c + 1) * n1].copy(), dist=dist[c * n1:(c + 1) * n1].copy(), hist=hist[c].copy(), ind=ind[c].copy())
    return res


def essential_graph_optimize(sim3, fixed, edge_v0, edge_v1, meas, fix_scale, n_iter=20, lambda_init=1e-16, pts=None, pt_ref=None,
                             device=0):
    """Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:785-1048) from initializeOptimization() to the corrected map
    points, on the device (qsp_essential_graph_optimize, include/qsp_hip.h).  sim3 (n_kf,8) tx ty tz qx qy qz qw s in hessian
    order; fixed (n_kf,) 1 = the vertex stays; edge_v0, edge_v1 (n_edge,) vertex indices and meas (n_edge,8) of the EdgeSim3 in
    insertion order; pts (n_pt,3) with pt_ref (n_pt,) the vertex index of each point's reference key frame, or None.
    Returns dict(sim3 (n_kf,8), pts (n_pt,3), iters, trace (iters,4): chi2, lambda, trials, last trial accepted)."""
    S0 = _arr(np.reshape(sim3, (-1, 8)), np.float64)
    n_kf = int(np.size(sim3)) // 8
    fx = _arr(np.reshape(fixed, -1), np.uint8)
    v0, v1 = _arr(np.reshape(edge_v0, -1), np.int32), _arr(np.reshape(edge_v1, -1), np.int32)
    n_edge = int(np.size(edge_v0))
    Z = _arr(np.reshape(meas, (-1, 8)), np.float64)
    if int(np.size(fixed)) != n_kf or int(np.size(edge_v1)) != n_edge or int(np.size(meas)) != 8 * n_edge:
        raise ValueError("essential_graph_optimize: array lengths do not agree")
    n_pt = 0 if pts is None else int(np.size(pts)) // 3
    if n_pt and (pt_ref is None or int(np.size(pt_ref)) != n_pt):
        raise ValueError("essential_graph_optimize: pt_ref must name one reference key frame per point")
    P = _arr(np.reshape(pts, (-1, 3)), np.float64) if n_pt else None
    R = _arr(np.reshape(pt_ref, -1), np.int32) if n_pt else None
    out, pout = np.zeros((n_kf, 8)), np.zeros((n_pt, 3))
    tr = _lib.EssentialTrace()
    _lib.check(_lib.lib().qsp_essential_graph_optimize(
        int(device), n_kf, _lib.dptr(S0), _lib.u8ptr(fx), n_edge, _lib.i32ptr(v0), _lib.i32ptr(v1), _lib.dptr(Z), 1 if fix_scale else 0,
        int(n_iter), float(lambda_init), n_pt, _lib.dptr(P) if n_pt else None, _lib.i32ptr(R) if n_pt else None, _lib.dptr(out),
        _lib.dptr(pout) if n_pt else None, C.byref(tr)))
    iters = int(tr.iters)
    trace = np.array(tr.trace[:], np.float64).reshape(32, 4)[:min(iters, 32)]
    return dict(sim3=out, pts=pout, iters=iters, trace=trace)


def essential_graph_stages(sim3, fixed, edge_v0, edge_v1, meas, fix_scale, lam, device=0):
    """One linearisation and one trial of essential_graph_optimize at `sim3` and the damping `lam`, every device buffer copied down
    (qsp_essential_graph_stages, include/qsp_hip.h): a window for tests.  Returns dict(E (n_edge,7), chi (n_edge,), J (n_edge,2,7,7)
    [edge][side][direction][error row], H (dim,dim), b (dim,), x (dim,), sim3_trial (n_kf,8), chi2, max_diag, chi2_trial, scale,
    failed, dim, nb)."""
    S0 = _arr(np.reshape(sim3, (-1, 8)), np.float64)
    n_kf = int(np.size(sim3)) // 8
    fx = _arr(np.reshape(fixed, -1), np.uint8)
    v0, v1 = _arr(np.reshape(edge_v0, -1), np.int32), _arr(np.reshape(edge_v1, -1), np.int32)
    n_edge = int(np.size(edge_v0))
    Z = _arr(np.reshape(meas, (-1, 8)), np.float64)
    if int(np.size(fixed)) != n_kf or int(np.size(edge_v1)) != n_edge or int(np.size(meas)) != 8 * n_edge:
        raise ValueError("essential_graph_stages: array lengths do not agree")
    dim = (6 if fix_scale else 7) * int(np.count_nonzero(fx == 0))
    E, chi, J = np.zeros((n_edge, 7)), np.zeros(n_edge), np.zeros((n_edge, 2, 7, 7))
    H, b, x, St, info = np.zeros((dim, dim)), np.zeros(dim), np.zeros(dim), np.zeros((n_kf, 8)), np.zeros(7)
    _lib.check(_lib.lib().qsp_essential_graph_stages(
        int(device), n_kf, _lib.dptr(S0), _lib.u8ptr(fx), n_edge, _lib.i32ptr(v0), _lib.i32ptr(v1), _lib.dptr(Z), 1 if fix_scale else 0,
        float(lam), *[_lib.dptr(a) for a in (E, chi, J, H, b, x, St, info)]))
    return dict(E=E, chi=chi, J=J, H=H, b=b, x=x, sim3_trial=St, chi2=float(info[0]), max_diag=float(info[1]), chi2_trial=float(info[2]),
                scale=float(info[3]), failed=float(info[4]), dim=int(info[5]), nb=int(info[6]))


class PlaceDatabase(object):
    """The key-frame database of place recognition, resident on the device (qsp_place_db, include/qsp_hip.h): the BoW vectors of
    every known key frame, which of them are listed (KeyFrameDatabase::add) in which order, and the reference's per-key-frame
    query state.  query() is KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates up to lScoreAndMatch
    (reference src/KeyFrameDatabase.cc:81-139 / :203-253), with DetectLoop's minimum score (src/LoopClosing.cc:131-148) when
    `ref_ids` is given; accumulate() is the covisibility pass over it (:144-196 / :258-308).  Bit for bit and in the reference's
    order.  words_hint / slots_hint: the initial capacities (they grow by doubling)."""
    LOOP, RELOC = 0, 1

    def __init__(self, device=0, words_hint=0, slots_hint=0):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().qsp_place_db_create(int(device), int(words_hint), int(slots_hint), C.byref(self._h)))

    def close(self):
        if self._h:
            _lib.lib().qsp_place_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _bow(words, values, who):
        if int(np.size(words)) != int(np.size(values)):
            raise ValueError("%s: one value per word" % who)
        return _arr(np.reshape(words, -1), np.int32), _arr(np.reshape(values, -1), np.float64), int(np.size(words))

    def put(self, kf_id, words, values, listed=True):
        w, v, n = self._bow(words, values, "PlaceDatabase.put")
        _lib.check(_lib.lib().qsp_place_db_put(self._h, int(kf_id), n, _lib.i32ptr(w), _lib.dptr(v), 1 if listed else 0))

    def list(self, kf_id):
        _lib.check(_lib.lib().qsp_place_db_list(self._h, int(kf_id)))

    def erase(self, kf_id):
        _lib.check(_lib.lib().qsp_place_db_erase(self._h, int(kf_id)))

    def clear(self):
        _lib.check(_lib.lib().qsp_place_db_clear(self._h))

    def size(self):
        """dict(known, listed, dead_slots, device_bytes)"""
        k, l, d, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().qsp_place_db_size(self._h, C.byref(k), C.byref(l), C.byref(d), C.byref(b)))
        return dict(known=k.value, listed=l.value, dead_slots=d.value, device_bytes=b.value)

    def query(self, mode, words, values, *, excluded=(), min_score=0.0, ref_ids=None, tap=True):
        """One query.  LOOP: `excluded` are the ids of the connected key frames; the minimum score is `min_score`, or computed from
        `ref_ids` (a non-empty list of known ids) as DetectLoop does.  Returns dict(n_sharing, max_common, min_common,
        min_score_used, match_id, match_score) -- lScoreAndMatch in the reference's order -- and, with tap, sharing_id,
        sharing_common, sharing_first: lKFsSharingWords in order."""
        w, v, n = self._bow(words, values, "PlaceDatabase.query")
        ex = _arr(np.reshape(np.asarray(excluded, np.int64), -1), np.int64)
        n_ex = int(np.size(excluded))
        n_ref = 0 if ref_ids is None else int(np.size(ref_ids))
        rf = _arr(np.reshape(np.asarray(ref_ids if n_ref else [], np.int64), -1), np.int64)
        cap = max(self.size()["listed"], 1)
        mid, ms = np.zeros(cap, np.int64), np.zeros(cap, np.float32)
        sid, sc, sf = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        i = _lib.PlaceQueryIn(int(mode), n, _lib.i32ptr(w), _lib.dptr(v), n_ex, _lib.i64ptr(ex), float(min_score), n_ref, _lib.i64ptr(rf))
        o = _lib.PlaceQueryOut(0, 0, 0, 0, 0.0, _lib.i64ptr(mid), _lib.fptr(ms), _lib.i64ptr(sid) if tap else None,
                               _lib.i32ptr(sc) if tap else None, _lib.i32ptr(sf) if tap else None)
        _lib.check(_lib.lib().qsp_place_db_query(self._h, C.byref(i), C.byref(o)))
        r = dict(n_sharing=int(o.n_sharing), max_common=int(o.max_common), min_common=int(o.min_common),
                 min_score_used=np.float32(o.min_score_used), match_id=mid[:o.n_match].copy(), match_score=ms[:o.n_match].copy())
        if tap:
            r.update(sharing_id=sid[:o.n_sharing].copy(), sharing_common=sc[:o.n_sharing].copy(), sharing_first=sf[:o.n_sharing].copy())
        return r

    def accumulate(self, mode, ids, neighbours):
        """The covisibility pass over the `match_id` the last query of `mode` returned.  neighbours: per entry the ids of
        GetBestCovisibilityKeyFrames(10), in order (a list of lists, or a callable id -> list).  Returns dict(cand_id, acc_score,
        best_id)."""
        n = int(np.size(ids))
        ids = _arr(np.reshape(np.asarray(ids, np.int64), -1), np.int64)
        nb = [list(neighbours(int(k))) for k in ids[:n]] if callable(neighbours) else [list(x) for x in neighbours]
        if len(nb) != n:
            raise ValueError("PlaceDatabase.accumulate: one neighbour list per entry")
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in nb])
        flat = _arr(np.array([k for x in nb for k in x], np.int64), np.int64)
        cand, acc, best = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int64)
        o = _lib.PlaceAccOut(0, _lib.i64ptr(cand), _lib.fptr(acc), _lib.i64ptr(best))
        _lib.check(_lib.lib().qsp_place_db_accumulate(self._h, int(mode), n, _lib.i64ptr(ids), _lib.i32ptr(off), _lib.i64ptr(flat),
                                                      C.byref(o)))
        return dict(cand_id=cand[:o.n_cand].copy(), acc_score=acc[:n].copy(), best_id=best[:n].copy())

    def _detect(self, mode, words, values, neighbours, **kw):
        q = self.query(mode, words, values, **kw)
        nb = neighbours if callable(neighbours) else [neighbours[int(k)] for k in q["match_id"]]
        q.update(self.accumulate(mode, q["match_id"], nb))
        return q

    def detect_loop_candidates(self, words, values, neighbours, *, excluded=(), min_score=0.0, ref_ids=None):
        """KeyFrameDatabase::DetectLoopCandidates: query + accumulate.  neighbours: a callable id -> ids of
        GetBestCovisibilityKeyFrames(10), or a table (dict) of them.  The candidates are `cand_id` of the returned dict."""
        return self._detect(self.LOOP, words, values, neighbours, excluded=excluded, min_score=min_score, ref_ids=ref_ids)

    def detect_relocalization_candidates(self, words, values, neighbours):
        """KeyFrameDatabase::DetectRelocalizationCandidates: query + accumulate, as detect_loop_candidates."""
        return self._detect(self.RELOC, words, values, neighbours)
