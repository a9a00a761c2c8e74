"""Seeded fixtures of the object-gate tests, shared by the CPU test of the restatement (tests/test_oracle_object_gate.py) and
the GPU test (tests/test_gpu_object_gate.py).  A case is the dict qsp_slam_amd.gate_object_points takes."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAND = 1e-5            # knife-edge distance below which a point's flag is left out of a comparison
LDS_POINTS = 4096      # QSP_GATE_LDS_POINTS; the GPU test checks it against the module's constant


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def cloud(seed, n, push=True):
    """normal(size=(n,3)) * [0.45, 0.16, 0.28] under a random rotation plus an offset of a few metres; for n > 10 two points
    are pushed 2.5 m away (in opposite directions) so that the erase pass has work"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3)) * np.array([0.45, 0.16, 0.28])
    x = x @ rotation(rng).T
    if push and n > 10:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        x[n // 3] += 2.5 * d
        x[(2 * n) // 3] -= 2.5 * d
    return (x + rng.uniform(-4.0, 4.0, size=3)).astype(np.float32)


# survivors and raw counts on both sides of every edge: 20 is where lo = int(0.05 N) steps to 1, 64 the wave, 256 the workgroup,
# LDS_POINTS the staging limit; two of the n > 10 points are erased, hence n and n + 2
PCA_SIZES = [1, 19, 20, 21, 22, 23, 63, 64, 65, 66, 67, 255, 256, 257, 258, 259, LDS_POINTS, LDS_POINTS + 1, LDS_POINTS + 3, 20000]


def pca_cases():
    c = {"n%d" % n: dict(pts_world=cloud(100 + n, n)) for n in PCA_SIZES}
    far = np.array([[0.0, 0.0, 0.0], [2.5, 0.0, 0.0]], np.float32) + np.float32(3.0)
    c["n2_all_erased"] = dict(pts_world=far)                              # both more than 1 m from their mean: BAD
    c["n0_empty"] = dict(pts_world=np.zeros((0, 3), np.float32))           # BAD
    rng = np.random.default_rng(7)
    t = np.round(cloud(8, 3000, push=False).astype(np.float64) * 8) / 8    # heavy ties: a 1/8 lattice, most points many times
    c["ties"] = dict(pts_world=t.astype(np.float32))
    z = rng.normal(size=(400, 3)) * np.array([0.45, 0.16, 0.28])           # about the origin: negative, zero and -0.0 coordinates
    z[::7, 0] = 0.0
    z[3::7, 1] = -0.0
    z[5::11, 2] = 0.0
    z[::13] = 0.0
    z[6::13] = -0.0
    c["signed_zeros"] = dict(pts_world=z.astype(np.float32))
    return c


def coplanar3():
    return dict(pts_world=np.array([[1.0, 2.0, 3.0], [1.3, 2.1, 3.0], [1.1, 2.4, 3.0]], np.float32))


def sim3(seed, scale):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = scale * rotation(rng)
    T[:3, 3] = rng.uniform(-3.0, 3.0, size=3)
    return T.astype(np.float32)


def mesh600():
    z = np.load(os.path.join(GOLDEN, "mc_lewiner_volumes.npz"))
    return z["decoder32_0_verts"][:600].copy()                  # float64 (600,3), as extract_meshes_from_codes returns it


def _points_about(T, verts, seed, n):
    """points spread over 1.6 x the mesh's box in the object frame, mapped to the world"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float32).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    xo = rng.uniform(-1.0, 1.0, size=(n, 3)) * 1.6 * np.maximum(np.abs(lo), np.abs(hi))
    T = T.astype(np.float64)
    return (xo @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def model_cases():
    c = {}
    m = mesh600()
    T = sim3(21, 1.7)
    c["mesh600"] = dict(pts_world=_points_about(T, m, 22, 2000), vertices=m, T_wo=T)
    c["verts10_skipped"] = dict(pts_world=_points_about(T, m, 23, 50), vertices=m[:10], T_wo=T)
    c["verts11"] = dict(pts_world=_points_about(T, m, 24, 300), vertices=m[:11].astype(np.float32), T_wo=T)
    # well inside and well outside each of the six scaled planes
    v = m.astype(np.float32).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    f = np.array([1.2, 1.5, 1.2])
    mid = (lo + hi) / 2
    probes, expect = [], []
    for ax in range(3):
        for bound in (f[ax] * lo[ax], f[ax] * hi[ax]):
            for k, inside in ((0.9, bound * 0.9), (1.1, bound * 1.1)):
                p = mid.copy()
                p[ax] = inside
                probes.append(p)
                expect.append(k > 1.0)
    Td = T.astype(np.float64)
    c["six_planes"] = dict(pts_world=(np.array(probes) @ Td[:3, :3].T + Td[:3, 3]).astype(np.float32), vertices=m, T_wo=T,
                           expect=np.array(expect))
    # ymin > 0: a factor on the coordinate (the reference) keeps points a factor on the extent would drop, and the reverse
    up = m.copy()
    up[:, 1] += 1.0 - up[:, 1].min() + 0.5                           # ymin = 1.5
    T2 = sim3(25, 0.8)
    c["ymin_positive"] = dict(pts_world=_points_about(T2, up, 26, 1500), vertices=up, T_wo=T2)
    c["model_large"] = dict(pts_world=_points_about(T, m, 27, LDS_POINTS + 5), vertices=m, T_wo=T)
    return c


def mixed_batch():
    """nine objects, PCA and MODEL interleaved, sizes from the lists above"""
    p, m = pca_cases(), model_cases()
    names = ["n65", "mesh600", "n1", "verts10_skipped", "n%d" % (LDS_POINTS + 1), "ymin_positive", "n0_empty", "model_large", "n257"]
    return [dict(p[k]) if k in p else {q: m[k][q] for q in ("pts_world", "vertices", "T_wo")} for k in names]
