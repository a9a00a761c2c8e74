"""Times qsp_fuse_batch on the GPU: one batched call over 1 / 20 / 100 targets of 2000 key points and a shared pool of 2000 map
points (every target lists the whole pool) against a loop of single-target calls through the same entry.  Median and min-max of
30 calls after warm-up, host wall clock around the whole call (struct building in Python, staging, upload, one launch, read-back).
The kernel's own time comes from a child run of the batched call under `rocprofv3 --kernel-trace` (no counters in that run).  The
reference's Fuse needs OpenCV and was not built or timed: no CPU comparison.

    python tools/time_fuse.py [n_target n_point n_kp] [--out FILE] [--commit TEXT]   (default: profiles/fuse.txt)"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_CALLS = 10


def scene(n_target, n_point, n_kp, seed=5):
    """a pool of n_point points in front of a base camera and n_target key frames near it (the pose overload, th = 3): a key point
    sits about half a pixel from the projection of each of the first n_kp points, every second one stereo"""
    from tests import search_sim3_oracle as so
    f32 = np.float32
    rng = np.random.default_rng(seed)
    K = so.CAM.astype(np.float64)
    uv = np.stack([rng.uniform(40, 600, n_point), rng.uniform(40, 440, n_point)], -1)
    z = rng.uniform(4.0, 8.0, n_point)
    Y = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)
    d = np.linalg.norm(Y, axis=1)
    level = rng.integers(1, 6, n_point)
    dist_max = (d * 1.2 ** (level + 0.5)).astype(f32)
    desc = rng.integers(0, 256, (n_point, 32)).astype(np.uint8)
    pool = dict(Xw=Y.astype(f32), normal=(Y / d[:, None]).astype(f32), dist_max=dist_max, dist_max_inv=f32(1.2) * dist_max,
                dist_min_inv=(f32(0.8) * dist_max / so.SF[-1]).astype(f32), desc=desc)
    targets = []
    for k in range(n_target):
        R, t = so._rot(rng, 0.02), rng.normal(size=3) * 0.08
        Yc = Y @ R.T + t
        kp = np.stack([K[0] * Yc[:, 0] / Yc[:, 2] + K[2], K[1] * Yc[:, 1] / Yc[:, 2] + K[3]], -1)
        kp = (np.resize(kp, (n_kp, 2)) + rng.normal(size=(n_kp, 2)) * 0.4).astype(f32)
        ur = np.resize(kp[:, 0] - 40.0 / np.resize(Yc[:, 2], n_kp), n_kp).astype(f32)
        ur[1::2] = -1.0
        targets.append(dict(bounds=so.BOUNDS_VGA, grid=so.GRID_VGA, log_scale=so.LOG_SCALE, scale_factors=so.SF.copy(), Rcw=R.astype(f32),
                            tcw=t.astype(f32), Ow=(-(R.T @ t)).astype(f32), K=np.array(list(so.CAM) + [40.0], f32), th=f32(3.0), kp=kp,
                            octave=(np.resize(level, n_kp) - (np.arange(n_kp) & 1)).astype(np.int32), desc=np.resize(desc, (n_kp, 32)),
                            u_right=ur, inv_level_sigma2=(f32(1) / (so.SF * so.SF)).astype(f32), check=True,
                            list=np.arange(n_point, dtype=np.int32)))
    return targets, pool


def kernel_time(shape):
    """microseconds of k_fuse_best per batched call: a fresh child under rocprofv3 --kernel-trace; None and the reason when the
    profiler is not there or leaves no trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in shape]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            return None, "the profiled child ran into its time limit"
        if r.returncode != 0:
            return None, "the profiled child ended with status %d" % r.returncode
        us = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "k_fuse_best" in row.get("Kernel_Name", ""):
                    us.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        if not us:
            return None, "no k_fuse_best dispatch in the trace"
        us = us[-CHILD_CALLS:]                           # the warm-up calls come first
        return (float(np.median(us)), min(us), max(us)), None


def main():
    from qsp_slam_amd.ba import fuse_batch
    argv, opt = sys.argv[1:], {}
    if argv and argv[0] == "--child":                   # the profiled run: the batched call only
        targets, pool = scene(*[int(v) for v in argv[1:4]])
        for _ in range(3 + CHILD_CALLS):
            fuse_batch(targets, pool)
        return
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "fuse.txt"))
    shapes = [tuple(int(v) for v in argv[:3])] if len(argv) >= 3 else [(nt, 2000, 2000) for nt in (1, 20, 100)]
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_fuse_batch, the pose overload (reprojection test on), th = 3, 640 x 480 on the 64 x 48 grid, 8 levels; every target lists the "
             "whole shared pool; the kernel is the brute-force stride over the target's key points (no cell index is built on the device; "
             "that form was not tried)",
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); "
             "kernel: k_fuse_best alone, from a child run of the batched call under rocprofv3 --kernel-trace, %d calls after 3 warm-up calls; "
             "measured with the library sources of commit %s" % (CHILD_CALLS, commit),
             "the two device forms compared are ONE batched call and a LOOP of single-target calls over the same inputs; the reference's "
             "Fuse (CPU, OpenCV) was not built or measured here: no speed-up over it is claimed", ""]

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    for shape in shapes:
        targets, pool = scene(*shape)
        matched = sum(int((r["best_idx"] >= 0).sum()) for r in fuse_batch(targets, pool))
        b = clock(lambda: fuse_batch(targets, pool))
        s = clock(lambda: [fuse_batch([t], pool) for t in targets])
        kt, why = kernel_time(shape)
        ktxt = "kernel %.0f (%.0f - %.0f)" % kt if kt else "kernel not measured: %s" % why
        lines.append("%3d targets x %d key points, pool of %d (%7d pairs, %6d matched):  one batched call %8.0f (%.0f - %.0f)   loop of single calls "
                     "%8.0f (%.0f - %.0f)   ratio %.2f   %s" % ((shape[0], shape[2], shape[1], shape[0] * shape[1], matched) + b + s + (s[0] / b[0], ktxt)))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
