"""Times qsp_sim3_ransac_batch on the GPU: one batched call over 1 / 4 / 16 loop candidates of 100 matches each at 300 iterations
against a loop of single-candidate calls over the same candidates.  Median and min-max of 50 calls after warm-up, host wall clock
around the whole call (uploads, two launches, read-back).  The reference's Sim3Solver was not timed: no CPU comparison.

    python tools/time_sim3_ransac.py [n_cand n_match] [--out FILE] [--commit TEXT]   (default: profiles/sim3_ransac.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from qsp_slam_amd.ba import sim3_ransac_batch
    from tests import sim3_ransac_oracle as so
    argv, opt = sys.argv[1:], {}
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "sim3_ransac.txt"))
    shapes = [(int(argv[0]), int(argv[1]))] if len(argv) >= 2 else [(1, 100), (4, 100), (16, 100)]
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_sim3_ransac_batch, 300 iterations per candidate, min_inliers = 20, fix_scale = 0, planted candidates (4 mm noise, three pairs in ten unrelated); "
             "every hypothesis is evaluated, the first success included (it lies within the first iterations on this data)",
             "host wall clock per call in microseconds, 50 calls after 5 warm-up calls: median (min - max); measured with the library sources of commit %s" % commit,
             "the reference's Sim3Solver (CPU, OpenCV) was not measured here: no CPU comparison is claimed", ""]

    def clock(fn):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(50):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    for nc, nm in shapes:
        cands = [so.make_candidate(100 + i, nm, "planted", 300, 0, swap=bool(i & 1)) for i in range(nc)]
        b = clock(lambda: sim3_ransac_batch(cands))
        s = clock(lambda: [sim3_ransac_batch([c]) for c in cands])
        lines.append("%2d candidates x %d matches:  one batched call %8.0f (%.0f - %.0f)   loop of single calls %8.0f (%.0f - %.0f)   ratio %.2f"
                     % ((nc, nm) + b + s + (s[0] / b[0],)))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
