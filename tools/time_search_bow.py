"""Times qsp_search_by_bow_batch on the GPU: one batched call over 16 loop candidates of 2000 key points with about 100 common
vocabulary nodes against 16 single-candidate calls, in both modes.  Median and min-max of 30 calls after warm-up, host wall clock
around the whole call (struct building in Python, the host-side checks, uploads, two launches, read-back).  The two kernels' own
times come from a child run of this script under `rocprofv3 --kernel-trace --stats` (skipped, and said so, where rocprofv3 is
missing), for the even scene and for one whose largest node holds a quarter of the key points: one wave walks a node serially,
so that node is the critical path of k_bow_match.  The reference's SearchByBoW needs OpenCV and DBoW2 and was not built or
timed: no CPU comparison.

    python tools/time_search_bow.py [n_cand n_kp] [--out FILE] [--commit TEXT]   (default: profiles/search_bow.txt)"""
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


def scene(n_cand, n_kp, n_nodes=100, big_share=0.0, seed=5):
    """the shared frame and n_cand candidates that see the same n_kp landmarks (a few descriptor bits flipped, turned by 40 degrees,
    seven in ten slots eligible); big_share of the landmarks fall into ONE node, the rest evenly over the others"""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    angle = rng.uniform(0, 360, n_kp).astype(np.float32)
    node = rng.integers(1, n_nodes, n_kp)
    node[rng.uniform(size=n_kp) < big_share] = 0

    def frame(perm, flips, rot):
        d = desc[perm].copy()
        for _ in range(flips):
            d[np.arange(n_kp), rng.integers(0, 32, n_kp)] ^= (1 << rng.integers(0, 8, n_kp)).astype(np.uint8)
        nd = node[perm]
        order = np.argsort(nd, kind="stable")                       # per node: ascending index, as DBoW2 fills the vector
        ids, counts = np.unique(nd, return_counts=True)
        return dict(desc=d, angle=((angle[perm] + rot + rng.normal(size=n_kp) * 3) % 360).astype(np.float32),
                    eligible=(rng.uniform(size=n_kp) < 0.7).astype(np.uint8), node_id=ids.astype(np.int32),
                    node_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), feat=order.astype(np.int32))

    shared = frame(np.arange(n_kp), 0, 0.0)
    return shared, [frame(rng.permutation(n_kp), 8, 40.0) for _ in range(n_cand)]


def largest_node(shared, cands):
    """(sources, targets, share of its candidate's descriptor pairs) of the node with the most pairs, over the candidates"""
    best = (0, 0, 0, 0.0)
    s_cnt = dict(zip(shared["node_id"].tolist(), np.diff(shared["node_off"]).tolist()))
    for c in cands:
        pairs = [(s_cnt.get(i, 0), n_t) for i, n_t in zip(c["node_id"].tolist(), np.diff(c["node_off"]).tolist())]
        total = sum(a * b for a, b in pairs)
        a, b = max(pairs, key=lambda p: p[0] * p[1])
        if a * b > best[2]:
            best = (a, b, a * b, a * b / max(total, 1))
    return best[0], best[1], best[3]


def kernel_times(shape, big_share):
    """mean duration in us of the two kernels in a child run under rocprofv3, or None"""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return None
    tmp = tempfile.mkdtemp(prefix="qsp_bow_prof_")
    try:
        subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                        "--child", str(shape[0]), str(shape[1]), str(big_share)], check=True, timeout=300, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        files = glob.glob(tmp + "/**/*kernel_stats.csv", recursive=True)
        if not files:
            return None
        out = {}
        for r in csv.DictReader(open(files[0])):
            for k in ("k_bow_match", "k_bow_rot"):
                if k in r["Name"]:
                    out[k] = (float(r["AverageNs"]) / 1e3, int(r["Calls"]))
        return out if len(out) == 2 else None
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    from qsp_slam_amd.ba import search_by_bow_batch
    argv, opt = sys.argv[1:], {}
    if argv and argv[0] == "--child":                   # the profiled run: 20 batched calls, nothing else
        shared, cands = scene(int(argv[1]), int(argv[2]), big_share=float(argv[3]))
        for _ in range(20):
            search_by_bow_batch(shared, cands)
        return
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "search_bow.txt"))
    nc, nk = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (16, 2000)
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_search_by_bow_batch, th = 50, nn_ratio = 0.75, orientation check on; every frame sees the same landmarks over about 100 "
             "vocabulary nodes, seven in ten slots eligible; one wave per (candidate, node of the source frame), one workgroup per candidate "
             "for the orientation check",
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); "
             "measured with the library sources of commit %s" % commit,
             "the two device forms compared are ONE batched call and a LOOP of single-candidate calls over the same inputs; the reference's "
             "SearchByBoW (CPU, OpenCV + DBoW2) was not built or measured here: no speed-up over it is claimed", ""]

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    shared, cands = scene(nc, nk)
    for sis, label, kw in ((True, "key-frame overload (loop closing) ", dict()), (False, "frame overload (relocalisation)  ", dict(th_inclusive=True))):
        sh = shared if sis else dict(shared, eligible=None)
        found = sum(r["n_matches"] for r in search_by_bow_batch(sh, cands, shared_is_source=sis, **kw))
        b = clock(lambda: search_by_bow_batch(sh, cands, shared_is_source=sis, **kw))
        s = clock(lambda: [search_by_bow_batch(sh, [c], shared_is_source=sis, **kw) for c in cands])
        lines.append("%s %2d candidates x %d key points (%5d matches):  one batched call %8.0f (%.0f - %.0f)   loop of single calls %8.0f (%.0f - %.0f)   ratio %.2f"
                     % ((label, nc, nk, found) + b + s + (s[0] / b[0],)))
    lines += ["", "the kernels' own times (rocprofv3 --kernel-trace --stats over 20 batched key-frame-overload calls, mean per launch in "
              "microseconds), for the even scene and for one whose largest node holds a quarter of the key points (that node's serial walk "
              "is one wave's work; it is NOT split, which would change the greedy):"]
    for share in (0.0, 0.25):
        sh, cs = scene(nc, nk, big_share=share)
        n_s, n_t, part = largest_node(sh, cs)
        kt = kernel_times((nc, nk), share)
        if kt is None:
            lines.append("largest node %4d sources x %4d targets = %.3f of its candidate's descriptor pairs:  kernel times not measured (rocprofv3 gave no kernel statistics here)"
                         % (n_s, n_t, part))
        else:
            lines.append("largest node %4d sources x %4d targets = %.3f of its candidate's descriptor pairs:  k_bow_match %8.1f   k_bow_rot %6.1f   (%d launches each)"
                         % (n_s, n_t, part, kt["k_bow_match"][0], kt["k_bow_rot"][0], kt["k_bow_match"][1]))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
