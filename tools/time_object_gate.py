#!/usr/bin/env python3
"""Times the object map-point gate (qsp_object_gates): one batched call over 1 / 16 / 64 objects of 2 000 points -- half PCA,
half MODEL with 600-vertex meshes -- against a loop of single-object calls over the same objects.  Wall clock around the
C-ABI call, which uploads, launches, synchronises and downloads, so a time is what a caller waits.  Median (min - max) ms per
call over `reps` repetitions after a warm-up; writes profiles/object_gate.txt.  The file is a record, not a bar.  The same clock
is then put around one ellipsoid plane fit (qsp_ellipsoid_fit_planes through its Python wrapper) of 1 / 16 / 64 ellipsoids.

usage: python tools/time_object_gate.py [reps] [--out FILE]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qsp_slam_amd import _lib, object_gate  # noqa: E402
from qsp_slam_amd.ellipsoid import optimize_ellipsoids_using_planes  # noqa: E402
from tests import object_gate_cases as GC  # noqa: E402


def flat_args(objs):
    """the flat arrays of object_gate.object_gates, prepared once so that only the library call is timed"""
    n = len(objs)
    model = ["vertices" in o for o in objs]
    pts = [o["pts_world"] for o in objs]
    verts = [np.asarray(o["vertices"], np.float32) if m else np.zeros((0, 3), np.float32) for o, m in zip(objs, model)]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in pts])
    vo = np.zeros(n + 1, np.int32)
    vo[1:] = np.cumsum([len(v) for v in verts])
    T = np.stack([o["T_wo"] if m else np.eye(4, dtype=np.float32) for o, m in zip(objs, model)])
    any_model = any(model)
    return (np.array(model, np.int32), off, np.concatenate(pts), T if any_model else None, vo if any_model else None,
            np.concatenate(verts) if any_model else None)


def timed(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return np.median(t), min(t), max(t)


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "object_gate.txt")
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    reps = int(argv[0]) if argv else 50
    if _lib.lib().qsp_device_count() < 1:
        raise SystemExit("no GPU visible: nothing is measured without one")
    mesh = GC.mesh600()
    lines = ["object map-point gate, qsp_object_gates: 2 000 points per object, PCA and MODEL (600 vertices) alternating",
             "wall clock around the call (upload + one launch + synchronise + download), %d repetitions after 3 warm-up calls" % reps,
             "median (min - max) ms per call", ""]
    for n in (1, 16, 64):
        objs = []
        for i in range(n):
            if i % 2 == 0:
                objs.append(dict(pts_world=GC.cloud(1000 + i, 2000)))
            else:
                T = GC.sim3(2000 + i, 1.7)
                objs.append(dict(pts_world=GC._points_about(T, mesh, 3000 + i, 2000), vertices=mesh, T_wo=T))
        batch = flat_args(objs)
        singles = [flat_args([o]) for o in objs]
        b = timed(lambda: object_gate.object_gates(*batch), reps)
        s = timed(lambda: [object_gate.object_gates(*a) for a in singles], reps)
        lines.append("%3d objects   one batched call %7.3f (%.3f - %.3f)   loop of %d single calls %7.3f (%.3f - %.3f)   ratio %.1fx"
                     % ((n,) + b + (n,) + s + (s[0] / b[0],)))
    lines += ["", "ellipsoid plane fit, qsp_ellipsoid_fit_planes: 12 noisy tangent planes per ellipsoid, 10 iterations, the same clock"]
    rng = np.random.default_rng(0)
    ells = np.concatenate([rng.normal(size=(64, 3)) + [0, 0, 3], np.tile([0.0, 0.0, 0.0, 1.0], (64, 1)), rng.uniform(0.2, 1.2, (64, 3))], axis=1)
    planes = []
    for e in ells:                                               # tangent planes of the axis-aligned ellipsoid, offsets jittered
        nrm = rng.normal(size=(12, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        planes.append(np.concatenate([nrm, (-nrm @ e[:3] - np.linalg.norm(nrm * e[7:], axis=1) + rng.normal(scale=0.01, size=12))[:, None]], axis=1))
    for n in (1, 16, 64):
        lines.append("%3d ellipsoids   one batched call %7.3f (%.3f - %.3f)" % ((n,) + timed(lambda: optimize_ellipsoids_using_planes(ells[:n], planes[:n]), reps)))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    with open(out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
