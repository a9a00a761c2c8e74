"""numpy restatement of the object map-point gate (qsp_object_gates): MapObject::RemoveOutliersSimple + ComputeCuboidPCA and
MapObject::RemoveOutliersModel of the reference, in two flavours --
  "f32": float32 throughout with the reference's sequential accumulation order (what the reference's binary evaluates, up to
         Eigen's product kernels),
  "f64": everything in double (what the device kernel approximates: double sums, one rounding at the end).
Both take the eigenvectors from np.linalg.eigh of the scatter in double and apply the library's sign convention: v2 enters
with its largest-magnitude component positive.  Each result also carries every point's knife-edge distance `edge`: how far
the point is from flipping a flag, so that a comparison can leave out the points no arithmetic can decide."""
import numpy as np

OK, BAD, SKIPPED = 0, 1, 2


def order_statistic(x, k):
    """the value std::sort leaves at index k (ties included): selection by counting, not by sorting"""
    x = np.asarray(x)
    for v in np.unique(x):
        if np.count_nonzero(x < v) <= k < np.count_nonzero(x <= v):
            return v
    raise ValueError("rank outside the array")


def _seq_sum(a, dt):
    """the sum a loop `s += a[i]` gives in dt (np.sum is pairwise)"""
    a = np.asarray(a, dt)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:], dt)
    return np.cumsum(a, axis=0, dtype=dt)[-1] if dt == np.float32 else a.sum(axis=0)


def _empty(n0, status, erased=None):
    return dict(status=status, erased=np.zeros(n0, bool) if erased is None else erased, outlier=np.zeros(n0, bool),
                whl=np.zeros(3), R=np.zeros((3, 3)), centre_w=np.zeros(3), T_wo=np.zeros((4, 4)), edge=np.full(n0, np.inf))


def pca_gate(pts_world, flavour="f64"):
    dt = np.float32 if flavour == "f32" else np.float64
    X0 = np.asarray(pts_world, np.float32).reshape(-1, 3).astype(dt)
    n0 = X0.shape[0]
    if n0 == 0:
        return _empty(0, BAD)
    mean0 = (_seq_sum(X0, dt) / dt(n0)).astype(dt)
    d0 = np.sqrt(((X0 - mean0) ** 2).sum(axis=1, dtype=dt)).astype(dt)
    erased = d0 > 1.0
    edge = np.abs(d0.astype(np.float64) - 1.0)
    X = X0[~erased]
    n = X.shape[0]
    if n == 0:
        r = _empty(n0, BAD, erased)
        r["edge"] = edge
        return r
    mean = (_seq_sum(X, dt) / dt(n)).astype(dt)
    Xs = (X - mean).astype(dt)
    cov = _seq_sum(Xs[:, :, None] * Xs[:, None, :], dt)
    _, V = np.linalg.eigh(cov.astype(np.float64))
    if V[np.argmax(np.abs(V[:, 2])), 2] < 0:
        V[:, 2] = -V[:, 2]
    V = V.astype(dt)
    R = np.stack([V[:, 1], V[:, 0], -V[:, 2]], axis=1)
    if np.linalg.det(R.astype(np.float64)) < 0:
        R[:, 0] = -R[:, 0]
    if R[1, 1] > 0:
        R[:, 0] = -R[:, 0]
        R[:, 1] = -R[:, 1]
    Rinv = np.linalg.inv(R).astype(dt)
    Xo = (X @ Rinv.T).astype(dt)                      # rows: R^-1 x
    lo, hi = int(0.05 * n), int(0.95 * n)
    xs = np.sort(Xo, axis=0)
    whl = (xs[hi] - xs[lo]).astype(dt)
    centre_o = ((xs[hi] + xs[lo]) / 2.0).astype(dt)
    centre_w = (R @ centre_o).astype(dt)
    if flavour == "f32":
        D = (Xo - (Rinv @ centre_w).astype(dt)).astype(dt)
        half = (np.float32(1.2) * whl / np.float32(2)).astype(dt)
    else:
        D = Xo - centre_o
        half = 1.2 * whl / 2.0
    out_s = (np.abs(D) > half).any(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(np.abs(D).astype(np.float64) - half.astype(np.float64))
        e = np.where(whl > 0, e / np.where(whl > 0, whl, 1).astype(np.float64), e)
    outlier = np.zeros(n0, bool)
    outlier[~erased] = out_s
    edge[~erased] = np.minimum(edge[~erased], e.min(axis=1))
    T = np.eye(4, dtype=dt)
    T[:3, :3] = (0.40 * np.float64(whl[2]) * R.astype(np.float64)).astype(dt) if flavour == "f64" else \
        (np.float32(0.40 * np.float64(whl[2])) * R).astype(dt)
    T[:3, 3] = centre_w
    return dict(status=OK, erased=erased, outlier=outlier, whl=whl.astype(np.float64), R=R.astype(np.float64),
                centre_w=centre_w.astype(np.float64), T_wo=T.astype(np.float64), edge=edge)


def model_gate(pts_world, T_wo, vertices, flavour="f64"):
    dt = np.float32 if flavour == "f32" else np.float64
    X = np.asarray(pts_world, np.float32).reshape(-1, 3).astype(dt)
    n0 = X.shape[0]
    V = np.zeros((0, 3), np.float32) if vertices is None else np.asarray(vertices).astype(np.float32).reshape(-1, 3)
    if V.shape[0] <= 10:
        return _empty(n0, SKIPPED)
    T = np.asarray(T_wo, np.float32).reshape(4, 4).astype(dt)
    vmin, vmax = V.min(axis=0).astype(dt), V.max(axis=0).astype(dt)
    M = T[:3, :3]
    scale = dt(np.cbrt(np.linalg.det(M.astype(np.float64))))
    whl = ((vmax - vmin) * scale).astype(dt)
    Minv = np.linalg.inv(M).astype(dt)
    if flavour == "f32":
        Xo = ((X @ Minv.T).astype(dt) - (Minv @ T[:3, 3]).astype(dt)).astype(dt)
    else:
        Xo = (X - T[:3, 3]) @ Minv.T
    f = np.array([1.2, 1.5, 1.2]).astype(dt)
    lo, hi = (f * vmin).astype(dt), (f * vmax).astype(dt)
    outlier = ((Xo > hi) | (Xo < lo)).any(axis=1)
    ext = (vmax - vmin).astype(np.float64)
    Xd = Xo.astype(np.float64)
    e = np.minimum(np.abs(Xd - hi.astype(np.float64)), np.abs(Xd - lo.astype(np.float64))) / ext
    r = _empty(n0, OK)
    r.update(outlier=outlier, whl=whl.astype(np.float64), edge=e.min(axis=1) if n0 else np.zeros(0))
    return r


def gate(obj, flavour="f64"):
    """obj: dict with "pts_world" and, for the mesh gate, "vertices" and "T_wo" (as qsp_slam_amd.gate_object_points takes it)"""
    if "vertices" in obj and "T_wo" in obj:
        return model_gate(obj["pts_world"], obj["T_wo"], obj["vertices"], flavour)
    return pca_gate(obj["pts_world"], flavour)
