"""The map-point gate of LocalMapping::ProcessDetectedObjects for every object of a key frame in one call
(qsp_object_gates, include/qsp_hip.h): MapObject::RemoveOutliersSimple + ComputeCuboidPCA (src/MapObject.cc:275-313, 361-475)
for objects without a mesh, MapObject::RemoveOutliersModel (src/MapObject.cc:316-358) for objects that have one."""
import numpy as np

from . import _lib
from .reconstruct.utils import ForceKeyErrorDict

GATE_PCA, GATE_MODEL = 0, 1
GATE_OK, GATE_BAD, GATE_SKIPPED = 0, 1, 2
LDS_POINTS = 4096          # QSP_GATE_LDS_POINTS: up to here an object's points are staged on chip
MAX_POINTS = 1 << 20       # QSP_GATE_MAX_POINTS


def object_gates(mode, pts_off, pts_world, T_wo=None, vert_off=None, verts=None, device=0):
    """The C-ABI call on flat arrays (see qsp_object_gate_in / _out).  Returns a dict of the seven output arrays."""
    mode = np.ascontiguousarray(mode, dtype=np.int32)
    pts_off = np.ascontiguousarray(pts_off, dtype=np.int32)
    n = mode.shape[0]
    pts = _lib.f32c(pts_world).reshape(-1, 3)
    gi = _lib.ObjectGateIn(n_obj=n, mode=_lib.i32ptr(mode), pts_off=_lib.i32ptr(pts_off), pts_world=_lib.fptr(pts))
    keep = [mode, pts_off, pts]
    if T_wo is not None:
        T = _lib.f32c(T_wo).reshape(-1, 4, 4)
        vo = np.ascontiguousarray(vert_off, dtype=np.int32)
        vv = _lib.f32c(verts).reshape(-1, 3)
        if vv.shape[0] == 0:
            vv = np.zeros((1, 3), np.float32)     # a pointer the library accepts; no vertex of it is read
        gi.T_wo, gi.vert_off, gi.verts = _lib.fptr(T), _lib.i32ptr(vo), _lib.fptr(vv)
        keep += [T, vo, vv]
    n_pt = int(pts_off[-1]) if n else 0
    out = dict(erased=np.zeros(n_pt, np.uint8), outlier=np.zeros(n_pt, np.uint8), whl=np.zeros((n, 3), np.float32),
               R=np.zeros((n, 3, 3), np.float32), centre_w=np.zeros((n, 3), np.float32), T_wo_pca=np.zeros((n, 4, 4), np.float32),
               status=np.zeros(n, np.int32))
    go = _lib.ObjectGateOut(erased=_lib.u8ptr(out["erased"]), outlier=_lib.u8ptr(out["outlier"]), whl=_lib.fptr(out["whl"]),
                            R=_lib.fptr(out["R"]), centre_w=_lib.fptr(out["centre_w"]), T_wo_pca=_lib.fptr(out["T_wo_pca"]),
                            status=_lib.i32ptr(out["status"]))
    _lib.check(_lib.lib().qsp_object_gates(int(device), gi, go))
    del keep
    return out


def _vertices_of(v):
    if isinstance(v, dict):                       # a result of refine_detections (a ForceKeyErrorDict)
        v = v["vertices"]
    elif not isinstance(v, np.ndarray) and hasattr(v, "vertices"):
        v = v.vertices
    if v is None:
        return np.zeros((0, 3), np.float32)
    return _lib.f32c(v).reshape(-1, 3)            # float64 -> float32 as .cast<Eigen::MatrixXf>() rounds


def gate_object_points(objects, device=0):
    """objects: a list of dicts.  "pts_world" (N,3), any dtype and stride: the world positions of the object's non-bad map points
    in GetMapPointsOnObject() order.  With "vertices" and "T_wo" the object is gated by its mesh (RemoveOutliersModel): vertices
    (V,3) float32 or float64, or a result of refine_detections(..., mesh_extractors=...) whose .vertices is taken (None: no
    vertex, the gate is skipped); T_wo (4,4) its Sim3Two.  Without them it gets the PCA cuboid (ComputeCuboidPCA).
    Returns one ForceKeyErrorDict per object: erased, outlier (N,) bool; w, h, l; R (3,3), centre_w (3,), T_wo (4,4) -- the pose
    ComputeCuboidPCA(true) would set; None for a mesh-gated object --; status (GATE_OK / GATE_BAD / GATE_SKIPPED)."""
    n = len(objects)
    if n == 0:
        return []
    pts = [_lib.f32c(o["pts_world"]).reshape(-1, 3) for o in objects]
    model = [("vertices" in o) and ("T_wo" in o) for o in objects]
    mode = np.array([GATE_MODEL if m else GATE_PCA for m in model], np.int32)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    flat = np.concatenate(pts, axis=0) if off[-1] else np.zeros((1, 3), np.float32)
    T = vo = vv = None
    if any(model):
        verts = [_vertices_of(o["vertices"]) if m else np.zeros((0, 3), np.float32) for o, m in zip(objects, model)]
        T = np.stack([_lib.f32c(o["T_wo"]).reshape(4, 4) if m else np.eye(4, dtype=np.float32) for o, m in zip(objects, model)])
        vo = np.zeros(n + 1, np.int32)
        vo[1:] = np.cumsum([v.shape[0] for v in verts])
        vv = np.concatenate(verts, axis=0)
    r = object_gates(mode, off, flat, T, vo, vv, device=device)
    out = []
    for i in range(n):
        s = slice(off[i], off[i + 1])
        pca = not model[i]
        out.append(ForceKeyErrorDict(erased=r["erased"][s].astype(bool), outlier=r["outlier"][s].astype(bool),
                                     w=float(r["whl"][i, 0]), h=float(r["whl"][i, 1]), l=float(r["whl"][i, 2]),
                                     R=r["R"][i].copy() if pca else None, centre_w=r["centre_w"][i].copy() if pca else None,
                                     T_wo=r["T_wo_pca"][i].copy() if pca else None, status=int(r["status"][i])))
    return out
