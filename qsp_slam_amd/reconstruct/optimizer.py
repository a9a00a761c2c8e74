"""Drop-in for reconstruct/optimizer.py of the reference: same class names, constructor and method signatures, return
types and failure behaviour; the numerics are batched HIP launches behind the C-ABI (include/qsp_hip.h).

Added on top of the reference interface (not replacing it): `reconstruct_objects_batched`, which runs many objects x
yaw-flip hypotheses in one resident batch -- what src/LocalMapping_util.cc:705-760 does as 4 serial Python calls per
object --, `OptimizerGroup`, the reference's per-class optimizers (src/LocalMapping.cc:33-69) refining the objects of
all classes in one batch over a decoder group, and `MeshExtractorGroup`, its per-class mesh extractors
(src/LocalMapping_util.cc:818-835) meshing the codes of all classes in one call."""
import ctypes as C
import math
import time

import numpy as np

from .. import _lib
from .utils import ForceKeyErrorDict


def _joint_cfg(o):
    return _lib.JointCfg(o.k1, o.k2, o.k3, o.k4, o.b1, o.b2, o.lr, o.s_damp, o.cut_off, int(o.num_iterations_joint_optim),
                         int(o.num_depth_samples), int(o.code_len))


def _flip_rotation(T, k, flip_angle):
    """T with its rotation block right-multiplied by Eigen::AngleAxisf(double(k) * flip_sample_angle, e_y).matrix()
    (src/LocalMapping_util.cc:722-726): the angle is narrowed to float before cos / sin, the (1,1) entry is (1-c)+c, and
    the 3x3 product sums over k in increasing order in float."""
    Tk = np.array(T, dtype=np.float32).reshape(4, 4).copy()
    if k == 0:
        return Tk
    f = np.float32
    a = float(f(float(k) * flip_angle))
    c, s = f(math.cos(a)), f(math.sin(a))
    Ry = np.array([[c, 0, s], [0, f(f(1) - c) + c, 0], [f(0) - s, 0, c]], dtype=np.float32)
    R = Tk[:3, :3].copy()
    for j in range(3):
        Tk[:3, j] = (R[:, 0] * Ry[0, j] + R[:, 1] * Ry[1, j]) + R[:, 2] * Ry[2, j]
    return Tk


def _is_group(decoder):
    from ..decoder import DecoderGroup
    return isinstance(decoder, DecoderGroup)


def _classes(decoder, n, obj_class):
    """the int32 class index array of a group call (None for a single decoder); range checks are the library's"""
    if not _is_group(decoder):
        if obj_class is not None:
            raise ValueError("obj_class needs a DecoderGroup")
        return None
    if obj_class is None or len(obj_class) != n:
        raise ValueError("a DecoderGroup needs one class index per object")
    return np.ascontiguousarray(obj_class, dtype=np.int32)


def _reconstruct_objects(decoder, cfg, pts, rays, depth, hyp_obj, t_cam_obj, code, obj_class=None):
    """qsp_reconstruct_objects: one call = fill + set_state + run + get on the batch that stays resident with the decoder (no device
    allocation per call once its capacities have settled) -- the reference's call pattern, src/LocalMapping_util.cc:705-760.
    decoder may be a DecoderGroup: then obj_class gives each object's class (qsp_reconstruct_objects_group)."""
    n_hyp = len(hyp_obj)
    L = decoder.code_len
    pts = [_lib.f32c(p).reshape(-1, 3) for p in pts]
    rays = [_lib.f32c(r).reshape(-1, 3) for r in rays]
    depth = [_lib.f32c(d).reshape(-1) for d in depth]
    n_pts = np.array([p.shape[0] for p in pts], np.int32)
    n_rays = np.array([r.shape[0] for r in rays], np.int32)
    n_fg = np.array([d.shape[0] for d in depth], np.int32)
    hyp = np.ascontiguousarray(hyp_obj, dtype=np.int32)
    pp, rp, dp = _lib.ptr_array(pts), _lib.ptr_array(rays), _lib.ptr_array(depth)
    T0 = _lib.f32c(t_cam_obj).reshape(n_hyp, 16)
    c0 = None if code is None else _lib.f32c(code).reshape(n_hyp, L)
    T = np.empty((n_hyp, 4, 4), np.float32)
    c = np.empty((n_hyp, L), np.float32)
    loss = np.empty(n_hyp, np.float32)
    good = np.empty(n_hyp, np.uint8)
    cls = _classes(decoder, len(pts), obj_class)
    head = (decoder.handle, C.byref(cfg), len(pts), C.cast(pp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_pts),
            C.cast(rp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_rays), C.cast(dp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_fg))
    tail = (n_hyp, _lib.i32ptr(hyp), _lib.fptr(T0), _lib.fptr(c0) if c0 is not None else _lib.c_float_p(), _lib.fptr(T), _lib.fptr(c),
            _lib.fptr(loss), _lib.u8ptr(good))
    if cls is None:
        _lib.check(_lib.lib().qsp_reconstruct_objects(*(head + tail)))
    else:
        _lib.check(_lib.lib().qsp_reconstruct_objects_group(*(head + (_lib.i32ptr(cls),) + tail)))
    return T, c, loss, good.astype(bool)


class RefineBatch(object):
    """Thin owner of a qsp_refine_batch* (resident device batch).  `decoder` may be a DecoderGroup: obj_class[o] is then the
    class (member index) of object o (qsp_refine_batch_create_group)."""

    def __init__(self, decoder, cfg, pts, rays, depth, hyp_obj, obj_class=None):
        L = _lib.lib()
        self.n_obj = len(pts)
        self.n_hyp = len(hyp_obj)
        self.code_len = decoder.code_len
        self._pts = [_lib.f32c(p).reshape(-1, 3) for p in pts]
        self._rays = [_lib.f32c(r).reshape(-1, 3) for r in rays]
        self._depth = [_lib.f32c(d).reshape(-1) for d in depth]
        n_pts = np.array([p.shape[0] for p in self._pts], np.int32)
        n_rays = np.array([r.shape[0] for r in self._rays], np.int32)
        n_fg = np.array([d.shape[0] for d in self._depth], np.int32)
        hyp = np.ascontiguousarray(hyp_obj, dtype=np.int32)
        pp, rp, dp = _lib.ptr_array(self._pts), _lib.ptr_array(self._rays), _lib.ptr_array(self._depth)
        h = C.c_void_p()
        cls = _classes(decoder, self.n_obj, obj_class)
        head = (decoder.handle, C.byref(cfg), self.n_obj, C.cast(pp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_pts),
                C.cast(rp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_rays), C.cast(dp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_fg))
        if cls is None:
            _lib.check(L.qsp_refine_batch_create(*(head + (self.n_hyp, _lib.i32ptr(hyp), C.byref(h)))))
        else:
            _lib.check(L.qsp_refine_batch_create_group(*(head + (_lib.i32ptr(cls), self.n_hyp, _lib.i32ptr(hyp), C.byref(h)))))
        self.handle = h
        self.decoder = decoder

    def set_state(self, t_cam_obj, code=None):
        T = _lib.f32c(t_cam_obj).reshape(self.n_hyp, 16)
        c = None if code is None else _lib.f32c(code).reshape(self.n_hyp, self.code_len)
        _lib.check(_lib.lib().qsp_refine_batch_set_state(self.handle, _lib.fptr(T), _lib.fptr(c) if c is not None
                                                         else _lib.c_float_p()))

    def run(self, n_iter=0):
        _lib.check(_lib.lib().qsp_refine_batch_run(self.handle, int(n_iter)))

    def get(self):
        T = np.empty((self.n_hyp, 4, 4), np.float32)
        code = np.empty((self.n_hyp, self.code_len), np.float32)
        loss = np.empty(self.n_hyp, np.float32)
        good = np.empty(self.n_hyp, np.uint8)
        _lib.check(_lib.lib().qsp_refine_batch_get(self.handle, _lib.fptr(T), _lib.fptr(code), _lib.fptr(loss),
                                                   _lib.u8ptr(good)))
        return T, code, loss, good.astype(bool)

    def trace(self):
        n = self.n_hyp
        H = np.empty((n, 71, 71), np.float32)
        b = np.empty((n, 71), np.float32)
        dx = np.empty((n, 71), np.float32)
        nv = np.empty(n, np.int32)
        nr = np.empty(n, np.int32)
        lt = np.empty((n, 2), np.float32)
        _lib.check(_lib.lib().qsp_refine_batch_trace(self.handle, _lib.fptr(H), _lib.fptr(b), _lib.fptr(dx),
                                                     _lib.i32ptr(nv), _lib.i32ptr(nr), _lib.fptr(lt)))
        return dict(H=H, b=b, dx=dx, n_valid=nv, K=nr, loss_sdf=lt[:, 0], loss_render=lt[:, 1])

    def trace_rot(self):
        """(n_hyp, 4): the rotation prior's J_rot (entries 3..5 of J_sim3) and res_rot of the last iteration (loss.py:155-178)"""
        r = np.empty((self.n_hyp, 4), np.float32)
        _lib.check(_lib.lib().qsp_refine_batch_trace_rot(self.handle, _lib.fptr(r)))
        return r

    def enable_rows(self, enable=True):
        _lib.check(_lib.lib().qsp_refine_batch_rows(self.handle, 1 if enable else 0, 0, _lib.c_float_p(),
                                                    _lib.c_float_p()))

    def rows(self, hyp, n_pts, n_render):
        """augmented Jacobian rows [J_pose(7) | J_code(64) | robust residual] of the last iteration (parity tests)"""
        a = np.empty((max(n_pts, 1), 72), np.float32)
        r = np.empty((max(n_render, 1), 72), np.float32)
        _lib.check(_lib.lib().qsp_refine_batch_rows(self.handle, 1, int(hyp), _lib.fptr(a), _lib.fptr(r)))
        return a[:n_pts], r[:n_render]

    def profile(self, enable=True):
        p = _lib.RefineProfile()
        _lib.check(_lib.lib().qsp_refine_batch_profile(self.handle, 1 if enable else 0, C.byref(p)))
        return p

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().qsp_refine_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Optimizer(object):
    """reconstruct/optimizer.py:26-281.  `decoder` is a qsp_slam_amd.decoder.DeepSdfDecoder."""

    def __init__(self, decoder, configs, debug=False):
        self.decoder = decoder
        optim_cfg = configs.optimizer
        self.k1 = optim_cfg.joint_optim.k1
        self.k2 = optim_cfg.joint_optim.k2
        self.k3 = optim_cfg.joint_optim.k3
        self.k4 = optim_cfg.joint_optim.k4
        self.b1 = optim_cfg.joint_optim.b1
        self.b2 = optim_cfg.joint_optim.b2
        self.lr = optim_cfg.joint_optim.learning_rate
        self.s_damp = optim_cfg.joint_optim.scale_damping
        self.num_iterations_joint_optim = optim_cfg.joint_optim.num_iterations
        self.code_len = optim_cfg.code_len
        self.num_depth_samples = optim_cfg.num_depth_samples
        self.cut_off = optim_cfg.cut_off_threshold
        self.debug = debug
        if configs.data_type == "KITTI":
            self.num_iterations_pose_only = optim_cfg.pose_only_optim.num_iterations

    # ---- reference entry point: one object, one hypothesis -----------------------------------------------------------
    def reconstruct_object(self, t_cam_obj, pts, rays, depth, code=None):
        """Same contract as the reference: returns an object with attrs t_cam_obj (4,4) f32 | None, code (L,) f32 | None,
        is_good, loss.  No exception for numeric failure."""
        r = self.reconstruct_objects_batched([dict(t_cam_obj=t_cam_obj, pts=pts, rays=rays, depth=depth, code=code)],
                                             flip_sample_num=1, select=False)
        return r[0][0]

    # ---- batched form: objects x yaw flips in one launch sequence ------------------------------------------------------
    def reconstruct_objects_batched(self, objects, flip_sample_num=1, select=True):
        """objects: list of dicts(t_cam_obj, pts, rays, depth, code=None).  For every object `flip_sample_num`
        hypotheses are refined: hypothesis k starts from t_cam_obj with its ROTATION BLOCK right-multiplied by
        R_y(k * 2pi / flip_sample_num) (src/LocalMapping_util.cc:713-726).
        select=False -> list (per object) of lists (per flip) of result objects;
        select=True  -> list (per object) of the result the reference's selection rule keeps
                        (LocalMapping_util.cc:748-752: replace if the kept one is not good, or if the new one is good
                        and has a smaller loss)."""
        return _reconstruct_batched(self, self.decoder, objects, flip_sample_num, select, None)

    # ---- the caller's loop around reconstruct_object, on the device ---------------------------------
    def refine_detections(self, detections, flip_sample_num=4, taps=False, mesh_extractor=None):
        """LocalMapping::ProcessDetectedObjects' marshalling + flip loop + keep rule (src/LocalMapping_util.cc:585-760) for a
        list of detections in ONE call (qsp_refine_detections, include/qsp_hip.h).  Each detection is a dict of WORLD-frame
        inputs, as the caller holds them:
            T_cw (4,4) key-frame pose, K (4,) fx fy cx cy, T_wo (4,4) Sim3Two of the map object, code (64,) | None,
            pts_world (M,3) map points on the object, fg_px (F,2) key-point pixels, fg_world (F,3) their map points,
            bg_rays (B,3), found_good_orientation (bool, default False -> flip_sample_num hypotheses, else one).
        Returns per detection the object the reference keeps in pyMapObjectLeastLoss (t_cam_obj None when not good), with
        the extra keys kept_flip and losses; taps=True adds the assembled pts / rays / depth / initial poses.
        mesh_extractor (a MeshExtractor of this optimizer's decoder): every result also carries .vertices and .faces, the mesh
        of its refined code -- what src/LocalMapping_util.cc:832-835 fetches next -- from one extract_meshes_from_codes call
        over the kept results; None for both on a result that was not kept or whose code has no surface."""
        out = _refine_detections(self, self.decoder, detections, flip_sample_num, taps, None)
        if mesh_extractor is not None:
            _attach_meshes(out, lambda codes, kept: mesh_extractor.extract_meshes_from_codes(codes))
        return out

    def estimate_pose_cam_obj(self, t_co_se3, scale, pts, code):
        """reconstruct/optimizer.py:47-93 -> (4,4) float32 SE3 (the reference returns a torch tensor that C++ casts to
        Eigen::Matrix4f, src/LocalMapping_util.cc:139-140; a numpy array casts the same way)."""
        return _estimate_pose(self, self.decoder, [dict(t_co_se3=t_co_se3, scale=scale, pts=pts, code=code)], None)[0]


def _reconstruct_batched(self, target, objects, flip_sample_num, select, classes):
    """Optimizer.reconstruct_objects_batched on `target` (a decoder, or a DecoderGroup with one class per object)"""
    n_obj = len(objects)
    hyp_obj, T0, codes = [], [], []
    any_code = any(o.get("code") is not None for o in objects)
    for i, o in enumerate(objects):
        T = np.asarray(o["t_cam_obj"], dtype=np.float32).reshape(4, 4)
        for k in range(flip_sample_num):
            Tk = _flip_rotation(T, k, 2.0 * math.pi / flip_sample_num)
            hyp_obj.append(i)
            T0.append(Tk)
            c0 = o.get("code")
            codes.append(np.zeros(self.code_len, np.float32) if c0 is None
                         else np.asarray(c0, np.float32)[: self.code_len])
    T, code, loss, good = _reconstruct_objects(target, _joint_cfg(self), [o["pts"] for o in objects],
                                               [o["rays"] for o in objects], [o["depth"] for o in objects], hyp_obj,
                                               np.stack(T0), np.stack(codes) if any_code else None, classes)
    out = []
    for i in range(n_obj):
        res = []
        for k in range(flip_sample_num):
            h = i * flip_sample_num + k
            if good[h]:
                res.append(ForceKeyErrorDict(t_cam_obj=T[h].copy(), code=code[h].copy(), is_good=True,
                                             loss=float(loss[h])))
            else:
                res.append(ForceKeyErrorDict(t_cam_obj=None, code=None, is_good=False, loss=float(loss[h])))
        if select:
            best = res[0]
            for r in res[1:]:
                if (not best.is_good) or (r.is_good and r.loss < best.loss):
                    best = r
            out.append(best)
        else:
            out.append(res)
    return out


def _refine_detections(self, target, detections, flip_sample_num, taps, classes):
    """Optimizer.refine_detections on `target` (a decoder, or a DecoderGroup with one class per detection)"""
    n = len(detections)
    f = _lib.f32c

    def cat(key, width):
        arrs = [f(d[key]).reshape(-1, width) for d in detections]
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in arrs])
        flat = np.concatenate(arrs, axis=0) if off[-1] else np.zeros((1, width), np.float32)
        return off, np.ascontiguousarray(flat)

    pts_off, pts_world = cat("pts_world", 3)
    fg_off, fg_px = cat("fg_px", 2)
    fg_off2, fg_world = cat("fg_world", 3)
    if not np.array_equal(fg_off, fg_off2):
        raise ValueError("fg_px and fg_world must have one row per feature point")
    bg_off, bg_rays = cat("bg_rays", 3)
    T_cw = f(np.stack([np.asarray(d["T_cw"], np.float32).reshape(4, 4) for d in detections]))
    T_wo = f(np.stack([np.asarray(d["T_wo"], np.float32).reshape(4, 4) for d in detections]))
    K = f(np.stack([np.asarray(d["K"], np.float32).reshape(4) for d in detections]))
    any_code = any(d.get("code") is not None for d in detections)
    code = f(np.stack([np.zeros(self.code_len, np.float32) if d.get("code") is None
                       else np.asarray(d["code"], np.float32)[: self.code_len] for d in detections]))
    n_flip = np.array([1 if d.get("found_good_orientation") else int(flip_sample_num) for d in detections], np.int32)
    n_hyp = int(n_flip.sum())
    inp = _lib.Detections(n, _lib.fptr(T_cw), _lib.fptr(K), _lib.fptr(T_wo),
                          _lib.fptr(code) if any_code else _lib.c_float_p(), _lib.i32ptr(n_flip),
                          2.0 * math.pi / float(flip_sample_num), _lib.i32ptr(pts_off), _lib.fptr(pts_world),
                          _lib.i32ptr(fg_off), _lib.fptr(fg_px), _lib.fptr(fg_world), _lib.i32ptr(bg_off),
                          _lib.fptr(bg_rays))
    T = np.empty((n, 4, 4), np.float32)
    c_out = np.empty((n, self.code_len), np.float32)
    loss = np.empty(n, np.float32)
    good = np.empty(n, np.uint8)
    kept = np.empty(n, np.int32)
    losses = np.empty(n_hyp, np.float32)
    res = _lib.DetectionResults(_lib.fptr(T), _lib.fptr(c_out), _lib.fptr(loss), _lib.u8ptr(good), _lib.i32ptr(kept),
                                _lib.fptr(losses))
    if taps:
        t_pts = np.empty((max(int(pts_off[-1]), 1), 3), np.float32)
        t_rays = np.empty((max(int(fg_off[-1] + bg_off[-1]), 1), 3), np.float32)
        t_depth = np.empty(max(int(fg_off[-1]), 1), np.float32)
        t_init = np.empty((n_hyp, 4, 4), np.float32)
        res.pts_cam, res.rays, res.depth_obs, res.t_cam_obj_init = (_lib.fptr(t_pts), _lib.fptr(t_rays),
                                                                    _lib.fptr(t_depth), _lib.fptr(t_init))
    if classes is None:
        _lib.check(_lib.lib().qsp_refine_detections(target.handle, C.byref(_joint_cfg(self)), C.byref(inp), C.byref(res)))
    else:
        cls = _classes(target, n, classes)
        _lib.check(_lib.lib().qsp_refine_detections_group(target.handle, C.byref(_joint_cfg(self)), C.byref(inp),
                                                          _lib.i32ptr(cls), C.byref(res)))
    out = []
    hyp_off = np.concatenate([[0], np.cumsum(n_flip)])
    ray_off = fg_off + bg_off
    for i in range(n):
        r = ForceKeyErrorDict(t_cam_obj=T[i].copy() if good[i] else None, code=c_out[i].copy() if good[i] else None,
                              is_good=bool(good[i]), loss=float(loss[i]), kept_flip=int(kept[i]),
                              losses=losses[hyp_off[i]:hyp_off[i + 1]].copy())
        if taps:
            r["pts"] = t_pts[pts_off[i]:pts_off[i + 1]].copy()
            r["rays"] = t_rays[ray_off[i]:ray_off[i + 1]].copy()
            r["depth"] = t_depth[fg_off[i]:fg_off[i + 1]].copy()
            r["t_cam_obj_init"] = t_init[hyp_off[i]:hyp_off[i + 1]].copy()
        out.append(r)
    return out


def _attach_meshes(results, extract):
    """.vertices / .faces on every result of a refine_detections call: the meshes extract(codes, kept) gives for the codes of the
    kept results (kept = their positions in the list), None for both everywhere else"""
    kept = [i for i, r in enumerate(results) if r.is_good]
    meshes = extract([results[i].code for i in kept], kept) if kept else []
    for r in results:
        r["vertices"] = r["faces"] = None
    for i, m in zip(kept, meshes):
        if m is not None:
            results[i]["vertices"], results[i]["faces"] = m.vertices, m.faces


def _estimate_pose(self, target, items, classes):
    """Optimizer.estimate_pose_cam_obj over a list of dicts(t_co_se3, scale, pts, code) in one call on `target` (a decoder, or
    a DecoderGroup with one class per item) -> list of (4,4) float32"""
    n = len(items)
    T = _lib.f32c(np.stack([np.asarray(it["t_co_se3"], np.float32).reshape(16) for it in items]))
    sc = np.array([it["scale"] for it in items], np.float32)
    ps = [_lib.f32c(it["pts"]).reshape(-1, 3) for it in items]
    n_pts = np.array([p.shape[0] for p in ps], np.int32)
    c = _lib.f32c(np.stack([np.asarray(it["code"], np.float32).reshape(-1)[: self.code_len] for it in items]))
    out = np.empty((n, 4, 4), np.float32)
    pp = _lib.ptr_array(ps)
    head = (target.handle, n, _lib.fptr(T), _lib.fptr(sc), C.cast(pp, C.POINTER(_lib.c_float_p)), _lib.i32ptr(n_pts), _lib.fptr(c))
    tail = (int(getattr(self, "num_iterations_pose_only", 5)), _lib.fptr(out))
    if classes is None:
        _lib.check(_lib.lib().qsp_estimate_pose(*(head + tail)))
    else:
        cls = _classes(target, n, classes)
        _lib.check(_lib.lib().qsp_estimate_pose_group(*(head + (_lib.i32ptr(cls),) + tail)))
    return [out[i] for i in range(n)]


class OptimizerGroup(object):
    """The reference's per-class optimizers (src/LocalMapping.cc:33-69: one Optimizer per class id of pSys->mmPyDecoders)
    refining the objects of ALL classes in one batch over a decoder group (include/qsp_hip.h, "Decoder groups") instead of
    one call per class.  `optimizers` = {class_id: Optimizer}; every object / detection dict carries a "class_id".  The
    reference assumes that all class decoders have the same code length and optimiser parameters (LocalMapping.cc:47): so
    does this class -- optimizers whose joint configs differ raise ValueError.  Results come back in input order."""

    def __init__(self, optimizers):
        if not optimizers:
            raise ValueError("OptimizerGroup needs at least one optimizer")
        self.class_ids = sorted(optimizers)
        self.optimizers = dict(optimizers)
        first = self.optimizers[self.class_ids[0]]

        def key(o):
            return (tuple(getattr(_joint_cfg(o), f[0]) for f in _lib.JointCfg._fields_),
                    int(getattr(o, "num_iterations_pose_only", 5)))
        for cid in self.class_ids[1:]:
            if key(self.optimizers[cid]) != key(first):
                raise ValueError("OptimizerGroup: the joint config of class %r differs from that of class %r (the classes of a "
                                 "group share code length and optimiser parameters)" % (cid, self.class_ids[0]))
        self._cfg = first
        self.code_len = first.code_len
        self._index = {cid: i for i, cid in enumerate(self.class_ids)}
        from ..decoder import DecoderGroup
        self.group = DecoderGroup([self.optimizers[cid].decoder for cid in self.class_ids])

    def _class_index(self, items, what):
        idx = []
        for i, it in enumerate(items):
            if "class_id" not in it:
                raise ValueError("%s %d has no \"class_id\"" % (what, i))
            cid = it["class_id"]
            if cid not in self._index:
                raise ValueError("%s %d: class_id %r has no optimizer in this group" % (what, i, cid))
            idx.append(self._index[cid])
        return np.array(idx, np.int32)

    def reconstruct_objects_batched(self, objects, flip_sample_num=1, select=True):
        """Optimizer.reconstruct_objects_batched over objects of several classes in one call"""
        cls = self._class_index(objects, "object")
        return _reconstruct_batched(self._cfg, self.group, objects, flip_sample_num, select, cls)

    def refine_detections(self, detections, flip_sample_num=4, taps=False, mesh_extractors=None):
        """Optimizer.refine_detections over the detections of several classes in one call: what LocalMapping_util.cc:585-760
        does per detection with the optimizer of its class.  mesh_extractors (a MeshExtractorGroup over the same class ids):
        every result also carries .vertices and .faces, the mesh of its refined code by the extractor of its class
        (LocalMapping_util.cc:818-835), from one group mesh call over the kept results; None for both on a result that was
        not kept or whose code has no surface."""
        cls = self._class_index(detections, "detection")
        out = _refine_detections(self._cfg, self.group, detections, flip_sample_num, taps, cls)
        if mesh_extractors is not None:
            _attach_meshes(out, lambda codes, kept: mesh_extractors.extract_meshes_from_codes(
                codes, [detections[i]["class_id"] for i in kept]))
        return out

    def estimate_pose_cam_obj(self, items):
        """Optimizer.estimate_pose_cam_obj for a list of dicts(t_co_se3, scale, pts, code, class_id) in one call -> list of (4,4)"""
        cls = self._class_index(items, "item")
        return _estimate_pose(self._cfg, self.group, items, cls)

    def close(self):
        self.group.close()


def create_voxel_grid(vol_dim=128):
    """reconstruct/utils.py:98-117, including its true-division quirk: `overall_index.long() / vol_dim` is a float
    division on torch >= 1.6, so the y and x coordinates keep their fractional part."""
    i = np.arange(vol_dim ** 3, dtype=np.int64)
    size = np.float32(2.0 / (vol_dim - 1))
    v = np.zeros((vol_dim ** 3, 3), np.float32)
    v[:, 2] = (i % vol_dim).astype(np.float32)
    v[:, 1] = np.mod((i / vol_dim).astype(np.float32), np.float32(vol_dim))
    v[:, 0] = np.mod((i / vol_dim).astype(np.float32) / np.float32(vol_dim), np.float32(vol_dim))
    return v * size - np.float32(1)


def split_batch_meshes(n_verts, n_faces, verts, faces, volumes=None):
    """The per-item results of a batch call from its concatenated arrays (qsp_mesh_fetch_batch): item i owns the next n_verts[i]
    rows of verts (sum V,3) and the next n_faces[i] rows of faces (sum F,3; indices local to the item's mesh), and volumes[i].
    Returns a list in item order of (vertices, faces, volume or None), copies that do not keep the batch's arrays alive -- or
    None for an item without a surface (n_verts[i] == 0)."""
    n_verts = np.asarray(n_verts, np.int64).reshape(-1)
    n_faces = np.asarray(n_faces, np.int64).reshape(-1)
    if len(n_verts) != len(n_faces):
        raise ValueError("n_verts and n_faces: one entry per item each")
    v_end, f_end = np.cumsum(n_verts), np.cumsum(n_faces)
    if len(n_verts) and (v_end[-1] != len(verts) or f_end[-1] != len(faces)):
        raise ValueError("the counts do not add up to the concatenated arrays")
    out = []
    for i in range(len(n_verts)):
        if n_verts[i] == 0:
            out.append(None)
            continue
        out.append((verts[v_end[i] - n_verts[i]:v_end[i]].copy(), faces[f_end[i] - n_faces[i]:f_end[i]].copy(),
                    None if volumes is None else volumes[i].copy()))
    return out


def _run_mesh_batch(handle, voxels_dim, n, volumes, call):
    """a batch call on the extractor `handle` -- call(n_verts*, n_faces*) -> status -- and the fetch of its result:
    split_batch_meshes' list"""
    nv, nf = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    _lib.check(call(_lib.i64ptr(nv), _lib.i64ptr(nf)))
    if n == 0:
        return []
    nv, nf = nv[:n], nf[:n]
    verts = np.empty((int(nv.sum()), 3), np.float64)
    faces = np.empty((int(nf.sum()), 3), np.int32)
    vols = np.empty((n,) + (voxels_dim,) * 3, np.float32) if volumes else None
    _lib.check(_lib.lib().qsp_mesh_fetch_batch(handle, None, verts.ctypes.data_as(C.POINTER(C.c_double)), _lib.i32ptr(faces),
                                               _lib.fptr(vols) if volumes else None))
    return split_batch_meshes(nv, nf, verts, faces, vols)


def _volume_rows(volumes, voxels_dim):
    """a sequence of (dim,dim,dim) volumes as the (n, dim^3) array the library reads, and n"""
    vols = [np.asarray(v, np.float32).reshape(-1) for v in volumes]
    if any(v.size != voxels_dim ** 3 for v in vols):
        raise ValueError("volumes must be (%d,)*3" % voxels_dim)
    return (_lib.f32c(np.stack(vols)) if vols else np.zeros(1, np.float32)), len(vols)


def _code_rows(codes, code_len, width):
    """a sequence of codes, each cut to code_len, as the zero-padded (n, width) array the library reads (width = the decoder's
    code length), and n"""
    rows = [np.asarray(c, np.float32).reshape(-1)[:code_len] for c in codes]
    host = np.zeros((max(len(rows), 1), width), np.float32)
    for i, c in enumerate(rows):
        host[i, :min(c.size, width)] = c[:width]
    return host, len(rows)


def _mesh_dicts(res, return_volumes):
    """split_batch_meshes' tuples as the objects extract_mesh_from_code returns (None stays None)"""
    out = []
    for r in res:
        if r is not None:
            d = ForceKeyErrorDict(vertices=r[0], faces=r[1])
            if return_volumes:
                d["sdf_volume"] = r[2]
            r = d
        out.append(r)
    return out


class MeshExtractor(object):
    """reconstruct/optimizer.py:284-304.  The SDF volume over create_voxel_grid(voxels_dim) is decoded and triangulated on
    the GPU (qsp_mesh_extract: MLP tile kernel + Lewiner's marching cubes, include/qsp_hip.h); only vertices and faces come
    back: vertices (V,3) float64 and faces (F,3) int32, the values and the order skimage.measure.marching_cubes_lewiner +
    convert_sdf_voxels_to_mesh (reconstruct/utils.py:120-141) give for the same volume.  Like there, a volume without a zero
    crossing raises (ValueError when 0 is outside its range, RuntimeError when no cell is crossed).
    method="table": the triangulation of rounds 2-3 (float32 vertices ordered by grid point; no exception for an empty mesh)."""

    def __init__(self, decoder, code_len=64, voxels_dim=64, method="lewiner"):
        if method not in ("lewiner", "table"):
            raise ValueError("method: 'lewiner' or 'table'")
        self.decoder = decoder
        self.code_len = code_len
        self.voxels_dim = voxels_dim
        self.method = method
        self.voxel_points = create_voxel_grid(vol_dim=self.voxels_dim)
        self.handle = C.c_void_p()
        pts = _lib.f32c(self.voxel_points)
        _lib.check(_lib.lib().qsp_mesh_extractor_create(decoder.handle, voxels_dim, _lib.fptr(pts), C.byref(self.handle)))
        _lib.check(_lib.lib().qsp_mesh_extractor_set_method(self.handle, 0 if method == "lewiner" else 1))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            _lib.lib().qsp_mesh_extractor_destroy(h)
            self.handle = C.c_void_p()

    def _fetch(self, nv, nf, volume=False):
        lewiner = self.method == "lewiner"
        verts = np.empty((nv.value, 3), np.float32)
        faces = np.empty((nf.value, 3), np.int32)
        want_vol = volume or (lewiner and nv.value == 0)
        vol = np.empty((self.voxels_dim,) * 3, np.float32) if want_vol else None
        _lib.check(_lib.lib().qsp_mesh_fetch(self.handle, _lib.fptr(verts), _lib.i32ptr(faces),
                                             _lib.fptr(vol) if want_vol else None))
        if lewiner:
            if nv.value == 0:      # skimage/measure/_marching_cubes_lewiner.py: the two ways an empty surface is reported
                if 0.0 < float(vol.min()) or 0.0 > float(vol.max()):
                    raise ValueError("Surface level must be within volume data range.")
                raise RuntimeError("No surface found at the given iso value.")
            verts = np.empty((nv.value, 3), np.float64)
            _lib.check(_lib.lib().qsp_mesh_fetch_f64(self.handle, verts.ctypes.data_as(C.POINTER(C.c_double))))
        return verts, faces, vol if volume else None

    def extract_sdf_grid(self, code):
        """(dim,dim,dim) SDF volume the reference hands to convert_sdf_voxels_to_mesh (optimizer.py:296-297)."""
        sdf = self.decoder.decode_sdf(np.asarray(code, np.float32)[: self.code_len], self.voxel_points)
        return sdf.reshape(self.voxels_dim, self.voxels_dim, self.voxels_dim)

    def mesh_from_volume(self, sdf_volume):
        """convert_sdf_voxels_to_mesh (reconstruct/utils.py:120-141) on a given (dim,dim,dim) volume."""
        vol = _lib.f32c(np.asarray(sdf_volume, np.float32).reshape(-1))
        if vol.size != self.voxels_dim ** 3:
            raise ValueError("volume must be (%d,)*3" % self.voxels_dim)
        nv, nf = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().qsp_mesh_from_volume(self.handle, _lib.fptr(vol), C.byref(nv), C.byref(nf)))
        verts, faces, _ = self._fetch(nv, nf)
        return verts, faces

    def extract_mesh_from_code(self, code, return_volume=False):
        start = time.time()
        code = _lib.f32c(np.asarray(code, np.float32)[: self.code_len])
        if code.size < 64:
            code = np.concatenate([code, np.zeros(64 - code.size, np.float32)])
        nv, nf = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().qsp_mesh_extract(self.handle, _lib.fptr(code), C.byref(nv), C.byref(nf)))
        verts, faces, vol = self._fetch(nv, nf, return_volume)
        print("Extract mesh takes %f seconds" % (time.time() - start))
        out = ForceKeyErrorDict(vertices=verts, faces=faces)
        if return_volume:
            out["sdf_volume"] = vol
        return out

    # ---- batches: many meshes per call (qsp_mesh_extract_batch / qsp_mesh_from_volumes, include/qsp_hip.h) ------------------
    def set_batch_limit(self, max_volumes_per_pass):
        """volumes a batch call holds scratch memory for at a time (1 .. 64, the default); results do not depend on it"""
        _lib.check(_lib.lib().qsp_mesh_extractor_set_batch_limit(self.handle, int(max_volumes_per_pass)))

    def _batch(self, entry, host, n, volumes):
        return _run_mesh_batch(self.handle, self.voxels_dim, n, volumes,
                               lambda nv, nf: entry(self.handle, n, _lib.fptr(host), nv, nf))

    def meshes_from_volumes(self, volumes):
        """mesh_from_volume on a sequence of (dim,dim,dim) volumes in one call: a list of (vertices, faces) in input order, the
        values mesh_from_volume gives for each -- or None for a volume without a surface, where the single call raises."""
        host, n = _volume_rows(volumes, self.voxels_dim)
        return [r if r is None else r[:2] for r in self._batch(_lib.lib().qsp_mesh_from_volumes, host, n, False)]

    def extract_meshes_from_codes(self, codes, return_volumes=False):
        """extract_mesh_from_code for a sequence of codes in one call (one grid decode and one marching-cubes launch chain for
        all of them, csrc/mesh_extract.hpp): a list, in input order, of the ForceKeyErrorDict(vertices (V,3) float64, faces (F,3)
        int32[, sdf_volume]) objects the single call returns, bit for bit (unless an fp16x2 range fallback repeats a pass on the f32
        pipe for items that alone would not have needed it).  Every code is cut to code_len and zero-padded as there.
        One difference: a code whose volume has no surface yields None at its place in the list -- the single call raises like
        scikit-image, which would lose the other meshes of the batch.  Lewiner's method only (method="table" is not batched)."""
        start = time.time()
        host, n = _code_rows(codes, self.code_len, self.decoder.code_len)
        res = self._batch(_lib.lib().qsp_mesh_extract_batch, host, n, return_volumes)
        print("Extract %d meshes takes %f seconds" % (n, time.time() - start))
        return _mesh_dicts(res, return_volumes)


class MeshExtractorGroup(object):
    """The reference's per-class mesh extractors (src/LocalMapping_util.cc:818-835: the MeshExtractor of the detection's class,
    mmPyMeshExtractors) meshing the codes of ALL classes in one call over a decoder group (qsp_mesh_extract_batch_group,
    include/qsp_hip.h) instead of one call per class.  `extractors` = {class_id: MeshExtractor}, the dictionary the embedder
    holds; a code's class index is the position of its class id among the sorted ids, as in OptimizerGroup.  The members share
    one voxel grid, so they must agree on voxels_dim, code_len and method: ValueError otherwise.  decoder_group: a DecoderGroup
    over the members' decoders in that order (an OptimizerGroup's .group) to use instead of building one; it is then the
    caller's to close.  Every item is bit for bit what extract_mesh_from_code of its class's extractor returns (the fp16x2
    range fallback repeats a pass for all classes in it: include/qsp_hip.h).  close() before the decoders go."""

    def __init__(self, extractors, decoder_group=None):
        if not extractors:
            raise ValueError("MeshExtractorGroup needs at least one extractor")
        self.class_ids = sorted(extractors)
        self.extractors = dict(extractors)
        first = self.extractors[self.class_ids[0]]
        for cid in self.class_ids[1:]:
            e = self.extractors[cid]
            for what in ("voxels_dim", "code_len", "method"):
                if getattr(e, what) != getattr(first, what):
                    raise ValueError("MeshExtractorGroup: %s of class %r differs from that of class %r (the classes of a group "
                                     "share one voxel grid)" % (what, cid, self.class_ids[0]))
        self.voxels_dim, self.code_len, self.method = first.voxels_dim, first.code_len, first.method
        self._index = {cid: i for i, cid in enumerate(self.class_ids)}
        self._own_group = decoder_group is None
        if decoder_group is None:
            from .. import decoder
            decoder_group = decoder.DecoderGroup([self.extractors[cid].decoder for cid in self.class_ids])
        self.group = decoder_group
        self._handle = None

    @property
    def handle(self):
        """the qsp_mesh_extractor* over the group, created at first use"""
        if self._handle is None:
            h = C.c_void_p()
            pts = _lib.f32c(create_voxel_grid(vol_dim=self.voxels_dim))
            _lib.check(_lib.lib().qsp_mesh_extractor_create_group(self.group.handle, self.voxels_dim, _lib.fptr(pts), C.byref(h)))
            self._handle = h
            _lib.check(_lib.lib().qsp_mesh_extractor_set_method(h, 0 if self.method == "lewiner" else 1))
        return self._handle

    def _class_index(self, class_ids, n):
        class_ids = list(class_ids)
        if len(class_ids) != n:
            raise ValueError("MeshExtractorGroup: %d class ids for %d codes (one per code)" % (len(class_ids), n))
        for i, cid in enumerate(class_ids):
            if cid not in self._index:
                raise ValueError("code %d: class_id %r has no extractor in this group" % (i, cid))
        return np.array([self._index[cid] for cid in class_ids], np.int32)

    def set_batch_limit(self, max_volumes_per_pass):
        """volumes a call holds scratch memory for at a time (1 .. 64, the default); results do not depend on it"""
        _lib.check(_lib.lib().qsp_mesh_extractor_set_batch_limit(self.handle, int(max_volumes_per_pass)))

    def extract_meshes_from_codes(self, codes, class_ids, return_volumes=False):
        """MeshExtractor.extract_meshes_from_codes over codes of several classes in one call: class_ids[i] is the class of
        codes[i].  A list in input order of ForceKeyErrorDict(vertices (V,3) float64, faces (F,3) int32[, sdf_volume]), None
        where a code's volume has no surface."""
        start = time.time()
        codes = list(codes)
        cls = self._class_index(class_ids, len(codes))
        host, n = _code_rows(codes, self.code_len, self.group.code_len)
        res = _run_mesh_batch(self.handle, self.voxels_dim, n, return_volumes,
                              lambda nv, nf: _lib.lib().qsp_mesh_extract_batch_group(self.handle, n, _lib.fptr(host), _lib.i32ptr(cls),
                                                                                    nv, nf))
        print("Extract %d meshes of %d classes takes %f seconds" % (n, len(self.class_ids), time.time() - start))
        return _mesh_dicts(res, return_volumes)

    def meshes_from_volumes(self, volumes):
        """MeshExtractor.meshes_from_volumes on the group's extractor (marching cubes alone: no class is involved)"""
        host, n = _volume_rows(volumes, self.voxels_dim)
        res = _run_mesh_batch(self.handle, self.voxels_dim, n, False,
                              lambda nv, nf: _lib.lib().qsp_mesh_from_volumes(self.handle, n, _lib.fptr(host), nv, nf))
        return [r if r is None else r[:2] for r in res]

    def close(self):
        """the extractor first, then the decoder group when this object built it"""
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            _lib.lib().qsp_mesh_extractor_destroy(h)
        self._handle = None
        if getattr(self, "_own_group", False) and getattr(self, "group", None) is not None:
            self.group.close()
        self.group = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
