"""Times qsp_search_for_triangulation_batch on the GPU: one batched call over 20 covisible neighbours of 2000 key points (about half
of the slots without a map point, about 100 common vocabulary nodes, the epipole inside the image) against 20 single-neighbour
calls, with only_stereo = 0 and check_orientation = 0 as LocalMapping::CreateNewMapPoints calls it.  Median and min-max of 30 calls
after warm-up, host wall clock around the whole call (struct building in Python, the host-side checks, one upload, two launches,
one read-back).  The two kernels' own times come from a child run of this script under `rocprofv3 --kernel-trace --stats` (skipped,
and said so, where rocprofv3 is missing), for the even scene and for one whose largest node holds a quarter of the key points.
The reference's SearchForTriangulation needs OpenCV and DBoW2 and was not built or timed: no CPU comparison.

    python tools/time_search_triangulation.py [n_cand n_kp] [--out FILE] [--commit TEXT]   (default: profiles/search_triangulation.txt)"""
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

FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0


def scene(n_cand, n_kp, n_nodes=100, big_share=0.0, seed=5):
    """key frame 1 at the origin and n_cand neighbours that moved mostly forward (the epipole stays inside the image) and see the
    same n_kp landmarks: half a pixel of noise per level, a few descriptor bits flipped, half of the slots without a map point,
    three in ten stereo; big_share of the landmarks fall into ONE node, the rest evenly over the others"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-4, 4, n_kp), rng.uniform(-3, 3, n_kp), rng.uniform(4, 14, n_kp)], 1)
    desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    node = rng.integers(1, n_nodes, n_kp)
    node[rng.uniform(size=n_kp) < big_share] = 0
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    Ki = np.linalg.inv(K)
    scale = 1.2 ** np.arange(8)

    def frame(perm, flips, R, t):
        d = desc[perm].copy()
        for _ in range(flips):
            d[np.arange(n_kp), rng.integers(0, 32, n_kp)] ^= (1 << rng.integers(0, 8, n_kp)).astype(np.uint8)
        Xc = X[perm] @ R.T + t
        octave = rng.integers(0, 8, n_kp)
        px = np.stack([FX * Xc[:, 0] / Xc[:, 2] + CX, FY * Xc[:, 1] / Xc[:, 2] + CY], 1) + rng.normal(size=(n_kp, 2)) * 0.5 * scale[octave][:, None]
        nd = node[perm]
        order = np.argsort(nd, kind="stable")                       # per node: ascending index, as DBoW2 fills the vector
        ids, counts = np.unique(nd, return_counts=True)
        return dict(desc=d, angle=rng.uniform(0, 360, n_kp).astype(np.float32), eligible=(rng.uniform(size=n_kp) < 0.5).astype(np.uint8),
                    node_id=ids.astype(np.int32), node_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                    feat=order.astype(np.int32), xy=px.astype(np.float32), stereo=(rng.uniform(size=n_kp) < 0.3).astype(np.uint8),
                    sigma2=(scale[octave] ** 2).astype(np.float32), scale=scale[octave].astype(np.float32))

    shared = frame(np.arange(n_kp), 0, np.eye(3), np.zeros(3))
    cands, F12, exy = [], [], []
    for _ in range(n_cand):
        w = rng.normal(size=3) * 0.03
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R2 = np.eye(3) + Wx + 0.5 * Wx @ Wx
        t2 = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 0.9)])
        cands.append(frame(rng.permutation(n_kp), 8, R2, t2))
        R12, t12 = R2.T, -R2.T @ t2
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        F12.append(Ki.T @ tx @ R12 @ Ki)
        exy.append([FX * t2[0] / t2[2] + CX, FY * t2[1] / t2[2] + CY])
    return shared, cands, np.array(F12, np.float32), np.array(exy, np.float32)


def largest_node(shared, cands):
    """(sources, targets) of the node with the most descriptor pairs, over the neighbours"""
    best = (0, 0)
    s_cnt = dict(zip(shared["node_id"].tolist(), np.diff(shared["node_off"]).tolist()))
    for c in cands:
        for i, n_t in zip(c["node_id"].tolist(), np.diff(c["node_off"]).tolist()):
            if s_cnt.get(i, 0) * n_t > best[0] * best[1]:
                best = (s_cnt.get(i, 0), n_t)
    return best


KERNELS = ("k_tri_match", "k_bow_rot")


def kernel_times(shape, big_share):
    """mean duration in us of the two kernels in a child run under rocprofv3, or None"""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return None
    tmp = tempfile.mkdtemp(prefix="qsp_tri_prof_")
    try:
        subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                        "--child", str(shape[0]), str(shape[1]), str(big_share)], check=True, timeout=300, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        files = glob.glob(tmp + "/**/*kernel_stats.csv", recursive=True)
        if not files:
            return None
        out = {}
        for r in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if k in r["Name"]:
                    out[k] = (float(r["AverageNs"]) / 1e3, int(r["Calls"]))
        return out if len(out) == 2 else None
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    from qsp_slam_amd.ba import search_for_triangulation_batch as search
    argv, opt = sys.argv[1:], {}
    if argv and argv[0] == "--child":                   # the profiled run: 20 batched calls, nothing else
        shared, cands, F12, exy = scene(int(argv[1]), int(argv[2]), big_share=float(argv[3]))
        for _ in range(20):
            search(shared, cands, F12, exy)
        return
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "search_triangulation.txt"))
    nc, nk = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (20, 2000)
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_search_for_triangulation_batch, th = 50, only_stereo = 0, check_orientation = 0 (as CreateNewMapPoints calls it); every key "
             "frame sees the same landmarks over about 100 vocabulary nodes, half of the slots without a map point, the epipole inside the "
             "image; one wave per (neighbour, position in key frame 1's feature list), one workgroup per neighbour for the tail",
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); "
             "measured with the library sources of commit %s" % commit,
             "the two device forms compared are ONE batched call and a LOOP of single-neighbour calls over the same inputs; the reference's "
             "SearchForTriangulation (CPU, OpenCV + DBoW2) was not built or measured here: no speed-up over it is claimed", ""]

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    for share, label in ((0.0, "even scene                     "), (0.25, "a quarter of the key points in one node")):
        shared, cands, F12, exy = scene(nc, nk, big_share=share)
        found = sum(r["n_matches"] for r in search(shared, cands, F12, exy))
        b = clock(lambda: search(shared, cands, F12, exy))
        s = clock(lambda: [search(shared, [c], F12[i:i + 1], exy[i:i + 1]) for i, c in enumerate(cands)])
        lines.append("%s %2d neighbours x %d key points (%5d matches):  one batched call %8.0f (%.0f - %.0f)   loop of single calls %8.0f (%.0f - %.0f)   loop / batched %.2f"
                     % ((label, nc, nk, found) + b + s + (s[0] / b[0],)))
    lines += ["", "the kernels' own times (rocprofv3 --kernel-trace --stats over 20 batched calls, mean per launch in microseconds), for the even "
              "scene and for one whose largest node holds a quarter of the key points (here a crowded node is MORE waves, one per source, "
              "each striding over the node's targets; it is not one wave's serial walk as in k_bow_match):"]
    for share in (0.0, 0.25):
        sh, cs, _, _ = scene(nc, nk, big_share=share)
        n_s, n_t = largest_node(sh, cs)
        kt = kernel_times((nc, nk), share)
        if kt is None:
            lines.append("largest node %4d sources x %4d targets:  kernel times not measured (rocprofv3 gave no kernel statistics here)" % (n_s, n_t))
        else:
            lines.append("largest node %4d sources x %4d targets:  k_tri_match %8.1f   k_bow_rot %6.1f   (%d launches each)"
                         % (n_s, n_t, kt["k_tri_match"][0], kt["k_bow_rot"][0], kt["k_tri_match"][1]))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
