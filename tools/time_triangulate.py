"""Times qsp_triangulate_batch and qsp_create_new_map_points_batch on the GPU.  The scene: 20 neighbours of 2000 key points
around a key frame of 2000; the match grid holds about 150 matches per neighbour (what SearchForTriangulation leaves) or a match in
every slot (the most the kernel can be given).  Reported, as host wall clock through the Python binding (struct building, staging,
upload, launches, read-back; median and min-max of 30 calls after 3 warm-up calls):
  - qsp_triangulate_batch in ONE call against 20 single-neighbour calls;
  - the chained call against search_for_triangulation_batch followed by triangulate_batch, on the scene of
    tools/time_search_triangulation.py with a plausible geometry beside it;
and the two new kernels' own times from a child run under `rocprofv3 --kernel-trace --stats` (no counters in that run).  The
reference's loop needs OpenCV and was not built or timed: no speed-up over it is claimed.

    python tools/time_triangulate.py [n_cand n_kp] [--out FILE] [--commit TEXT]   (default: profiles/triangulate.txt;
    TEXT names the sources where no git metadata travels with the tree, e.g. "commit 1a2b3c4")"""
import csv
import glob
import importlib.util
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
KERNELS = ("k_tri_points", "k_tri_first")


def scene(n_cand, n_kp, per_neighbour, seed=11):
    """key frame 1 and n_cand neighbours 0.2 to 1 m away that see the same n_kp landmarks at 2 to 10 m, half of the slots stereo;
    per_neighbour matches per neighbour, nine in ten of them right (None: every slot matched)"""
    from tests import triangulate_oracle as to
    rng = np.random.RandomState(seed)
    kf1 = to.frame(to._rot([0.01, -0.02, 0.01]), [0.0, 0.0, 0.0], 520.0, 520.0, 320.0, 240.0, 0.1, 8, 1.2)
    depth = rng.uniform(2, 10, n_kp)
    px = np.stack([rng.uniform(20, 620, n_kp), rng.uniform(20, 460, n_kp)], -1)
    pc = np.stack([(px[:, 0] - 320.0) / 520.0 * depth, (px[:, 1] - 240.0) / 520.0 * depth, depth], -1)
    Xw = (pc - kf1["tcw"].astype(np.float64)) @ kf1["Rcw"].astype(np.float64)
    octave = rng.randint(0, 8, n_kp)
    to._observe(kf1, Xw, rng.rand(n_kp) < 0.5, octave, rng, 0.4)
    kf2s, match = [], np.full((n_cand, n_kp), -1, np.int32)
    for k in range(n_cand):
        fr = to.frame(to._rot(rng.normal(size=3) * 0.03), rng.uniform(-1, 1, 3) * [1.0, 0.3, 0.5], 520.0, 520.0, 320.0, 240.0, 0.1, 8, 1.2)
        perm = rng.permutation(n_kp)                                   # slot j of the neighbour sees landmark perm[j]
        to._observe(fr, Xw[perm], rng.rand(n_kp) < 0.5, octave[perm], rng, 0.4)
        inv = np.argsort(perm)
        who = np.arange(n_kp) if per_neighbour is None else rng.permutation(n_kp)[:per_neighbour]
        match[k, who] = inv[who]
        wrong = who[rng.rand(len(who)) < 0.1]
        match[k, wrong] = rng.randint(0, n_kp, len(wrong))
        kf2s.append(fr)
    return kf1, kf2s, match


def chained_scene(n_cand, n_kp):
    from tests import triangulate_oracle as to
    spec = importlib.util.spec_from_file_location("time_search_triangulation", os.path.join(ROOT, "tools", "time_search_triangulation.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    shared, cands, F12, exy = ts.scene(n_cand, n_kp)
    return to.with_geometry(shared, 0), [to.with_geometry(c, 1 + i) for i, c in enumerate(cands)], F12, exy


def kernel_times(shape):
    """name -> (median, min, max) microseconds per dispatch, from a fresh child under rocprofv3; None and the reason otherwise"""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in shape]
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
        if not all(us.values()):
            return None, "no dispatch of the kernels in the trace"
        return {k: (float(np.median(v[-CHILD_CALLS:])), min(v[-CHILD_CALLS:]), max(v[-CHILD_CALLS:])) for k, v in us.items()}, None


def main():
    from qsp_slam_amd.ba import create_new_map_points_batch, search_for_triangulation_batch, triangulate_batch
    argv, opt = sys.argv[1:], {}
    if argv and argv[0] == "--child":                   # the profiled run: the batched call on the full grid only
        kf1, kf2s, match = scene(int(argv[1]), int(argv[2]), None)
        for _ in range(3 + CHILD_CALLS):
            triangulate_batch(kf1, kf2s, match)
        return
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "triangulate.txt"))
    n_cand, n_kp = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (20, 2000)
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = "commit " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "an unknown commit (no git metadata here)"
    lines = ["qsp_triangulate_batch and qsp_create_new_map_points_batch: %d neighbours of %d key points, key frame 1 of %d; half of the slots "
             "stereo; one lane per (neighbour, slot), FP64 Jacobi on the SVD path" % (n_cand, n_kp, n_kp),
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); kernels: "
             "from a child run of the batched call on the full grid under rocprofv3 --kernel-trace --stats, %d calls after 3 warm-up calls; "
             "measured with the library sources of %s" % (CHILD_CALLS, commit),
             "compared are device forms only; the reference's loop (CPU, OpenCV) was not built or measured here: no speed-up over it is claimed", ""]

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    for label, per in (("about 150 matches per neighbour", 150), ("every slot matched", None)):
        kf1, kf2s, match = scene(n_cand, n_kp, per)
        res = triangulate_batch(kf1, kf2s, match)
        b = clock(lambda: triangulate_batch(kf1, kf2s, match))
        s = clock(lambda: [triangulate_batch(kf1, [f], match[k:k + 1]) for k, f in enumerate(kf2s)])
        lines.append("triangulation, %s (%d matches, %d accepted, %d new points):  one batched call %8.0f (%.0f - %.0f)   loop of single calls "
                     "%8.0f (%.0f - %.0f)   ratio %.2f" % ((label, int((match >= 0).sum()), sum(int(r["accept"].sum()) for r in res),
                                                           sum(r["n_new"] for r in res)) + b + s + (s[0] / b[0],)))
    kf1, kf2s, F12, exy = chained_scene(n_cand, n_kp)
    found = search_for_triangulation_batch(kf1, kf2s, F12, exy)

    def two_calls():
        f = search_for_triangulation_batch(kf1, kf2s, F12, exy)
        return triangulate_batch(kf1, kf2s, np.stack([r["match"] for r in f]))
    c = clock(lambda: create_new_map_points_batch(kf1, kf2s, F12, exy))
    t = clock(two_calls)
    lines.append("search and triangulation (%d matches):  the chained call %8.0f (%.0f - %.0f)   the two calls %8.0f (%.0f - %.0f)   ratio %.2f"
                 % ((sum(r["n_matches"] for r in found),) + c + t + (t[0] / c[0],)))
    kt, why = kernel_times((n_cand, n_kp))
    lines.append("kernels, every slot matched:  " + ("   ".join("%s %.0f (%.0f - %.0f)" % ((k,) + kt[k]) for k in KERNELS) if kt else "not measured: %s" % why))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
