"""Times qsp_search_by_projection_kf on the GPU: one call at 2000 key points with 1000 RELOC sources (Tracking::Relocalization) at
(th 10, ORBdist 100) and at (th 3, ORBdist 64), and with 2000 and 8000 SIM3 sources (LoopClosing::ComputeSim3, th 10), on synthetic
scenes of the kind tools/time_fuse.py uses.  Median and min-max of 30 calls after warm-up, host wall clock around the whole call
(struct building in Python, staging, upload, the gate launch, one round launch and one 4-byte read-back per round, download, the
action phase on the host), the number of rounds, and the two kernels' own times from a fresh child process under `rocprofv3
--kernel-trace` (no counters in that run).  There is no earlier device form to compare with, and the reference's functions need
OpenCV and were not built or timed: no speed-up is claimed.

    python tools/time_search_projection_kf.py [--out FILE] [--commit TEXT]   (default: profiles/search_projection_kf.txt)"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
CHILD_CALLS = 10
SHAPES = (("reloc", 1000, 2000, 10.0, 100), ("reloc", 1000, 2000, 3.0, 64), ("sim3", 2000, 2000, 10.0, 50), ("sim3", 8000, 2000, 10.0, 50))
KERNELS = ("k_proj_gate_kf", "k_proj_round")


def scene(mode, n_src, n_kp, th, orb_dist, seed=5):
    """time_fuse's scene with one frame: a key point about half a pixel from the projection of each of the first n_kp sources, a
    fifth of the slots taken at entry; RELOC with the orientation check"""
    import time_fuse
    f32 = np.float32
    targets, pool = time_fuse.scene(1, n_src, n_kp, seed)
    rng = np.random.default_rng(seed + 1)
    T = targets[0]
    frame = dict(T, slot_blocked=(rng.random(n_kp) < 0.2).astype(np.uint8), kp_angle=rng.uniform(0, 360, n_kp).astype(f32))
    src = dict(pool, valid=np.ones(n_src, np.uint8), angle=np.resize(frame["kp_angle"], n_src).astype(f32))
    return frame, src, dict(mode=mode, th=th, orb_dist=orb_dist, check_orientation=mode == "reloc")


def kernel_times(shape):
    """microseconds per call of each kernel (k_proj_round: all rounds of a call summed): a fresh child under rocprofv3
    --kernel-trace; None and the reason when the profiler is not there or leaves no trace"""
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
        us = {k: [] for k in KERNELS}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in KERNELS:
                    if k in row.get("Kernel_Name", ""):
                        us[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        if not us[KERNELS[0]] or not us[KERNELS[1]]:
            return None, "no dispatch of the kernels in the trace"
        calls = len(us[KERNELS[0]])
        return {k: sum(v) / calls for k, v in us.items()}, None


def main():
    from qsp_slam_amd.ba import search_by_projection_kf
    argv, opt = sys.argv[1:], {}
    if argv and argv[0] == "--child":                   # the profiled run
        frame, src, o = scene(argv[1], int(argv[2]), int(argv[3]), float(argv[4]), int(argv[5]))
        for _ in range(3 + CHILD_CALLS):
            search_by_projection_kf(frame, src, **o)
        return
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "search_projection_kf.txt"))
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_search_by_projection_kf on SYNTHETIC scenes: 640 x 480 on the 64 x 48 grid, 8 levels, one key point near the projection of each "
             "of the first 2000 sources, a fifth of the slots taken at entry; RELOC with the orientation check",
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); "
             "kernels: microseconds per call from a child run under rocprofv3 --kernel-trace (k_proj_round: all rounds of a call summed), "
             "%d calls after 3 warm-up calls; measured with the library sources of commit %s" % (CHILD_CALLS, commit),
             "there is no earlier device form of these functions and the reference's (CPU, OpenCV) was not built or measured here: no "
             "speed-up is claimed.  Each round costs one launch and one 4-byte read-back.  The round counts below are those of THESE synthetic "
             "scenes; round counts on real sequences are unmeasured", ""]
    for shape in SHAPES:
        frame, src, o = scene(*shape)
        res = search_by_projection_kf(frame, src, **o)
        for _ in range(3):
            search_by_projection_kf(frame, src, **o)
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            search_by_projection_kf(frame, src, **o)
            ts.append((time.perf_counter() - t) * 1e6)
        kt, why = kernel_times(shape)
        ktxt = "k_proj_gate_kf %.0f, k_proj_round %.0f" % (kt[KERNELS[0]], kt[KERNELS[1]]) if kt else "kernels not measured: %s" % why
        lines.append("%-5s %4d sources x %d key points, th %2.0f, accept <= %3d (%4d matches):  %d rounds   one call %8.0f (%.0f - %.0f)   %s"
                     % (shape[0].upper(), shape[1], shape[2], shape[3], shape[4], res["n_matches"], res["n_rounds"], np.median(ts), min(ts), max(ts), ktxt))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
