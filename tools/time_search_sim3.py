"""Times qsp_search_by_sim3_batch on the GPU: one batched call over 1 / 4 / 16 loop candidates of 1000 and 2000 key points per frame
against a loop of single-candidate calls over the same candidates.  Median and min-max of 30 calls after warm-up, host wall clock
around the whole call (struct building in Python, uploads, two launches, read-back).  The reference's SearchBySim3 needs OpenCV
and was not built or timed: no CPU comparison.

    python tools/time_search_sim3.py [n_cand n_kp] [--out FILE] [--commit TEXT]   (default: profiles/search_sim3.txt)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n_cand, n_kp, seed=5):
    """key frame 1 and n_cand key frames 2 of n_kp key points each: seven in ten slots hold a point both frames see"""
    from tests import search_sim3_oracle as so
    rng = np.random.default_rng(seed)
    R1, t1 = so._rot(rng, 0.4), rng.normal(size=3) * 0.5
    uv = np.stack([rng.uniform(20, 620, n_kp), rng.uniform(20, 460, n_kp)], -1)
    Y = np.stack([so._unpix(uv[i], rng.uniform(3.0, 8.0)) for i in range(n_kp)])
    desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    level = rng.integers(1, so.N_LEVELS - 1, n_kp)

    def frame(R, t, Yc, perm):
        fr = dict(bounds=so.BOUNDS_VGA, grid=so.GRID_VGA, log_scale=so.LOG_SCALE, scale_factors=so.SF.copy(), Rcw=R.astype(np.float32),
                  tcw=t.astype(np.float32), **so._mp_fields(n_kp))
        kp, octave, de = np.zeros((n_kp, 2), np.float32), np.zeros(n_kp, np.int32), np.zeros((n_kp, 32), np.uint8)
        Rd, td = fr["Rcw"].astype(np.float64), fr["tcw"].astype(np.float64)
        for j, i in enumerate(perm):
            so._set_point(fr, j, Yc[i], int(level[i]), desc[i], Rd, td)
            kp[j] = so._pix(Yc[i]) + rng.normal(size=2) * 0.7
            octave[j] = level[i] - (j & 1)
            de[j] = desc[i]
            fr["has_point"][j] = j % 10 < 7
        fr.update(kp=kp, octave=octave, desc=de)
        return fr

    kf1 = frame(R1, t1, Y, np.arange(n_kp))
    cands = []
    for c in range(n_cand):
        s12, R12, t12, R2, t2 = so._sim3(500 + c)
        Z = np.stack([so._to_cam2(s12, R12, t12, y) for y in Y])
        cands.append(dict(kf2=frame(R2, t2, Z, rng.permutation(n_kp)), K=so.CAM.copy(), s12=np.float32(s12), R12=R12.astype(np.float32),
                          t12=t12.astype(np.float32), th=np.float32(7.5)))
    return kf1, cands


def main():
    from qsp_slam_amd.ba import search_by_sim3_batch
    argv, opt = sys.argv[1:], {}
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "search_sim3.txt"))
    shapes = [(int(argv[0]), int(argv[1]))] if len(argv) >= 2 else [(nc, nk) for nk in (1000, 2000) for nc in (1, 4, 16)]
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_search_by_sim3_batch, th = 7.5, 640 x 480 on the 64 x 48 grid, 8 levels; seven in ten slots of either frame hold a map point "
             "both frames see; the kernel is the brute-force stride over the target's key points (no grid is built on the device; that form "
             "was not tried)",
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); "
             "measured with the library sources of commit %s" % commit,
             "the two device forms compared are ONE batched call and a LOOP of single-candidate calls over the same inputs; the reference's "
             "SearchBySim3 (CPU, OpenCV) was not built or measured here: no speed-up over it is claimed", ""]

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    for nc, nk in shapes:
        kf1, cands = scene(nc, nk)
        found = sum(r["n_found"] for r in search_by_sim3_batch(kf1, cands))
        b = clock(lambda: search_by_sim3_batch(kf1, cands))
        s = clock(lambda: [search_by_sim3_batch(kf1, [c]) for c in cands])
        lines.append("%2d candidates x %d key points (%5d matches found):  one batched call %8.0f (%.0f - %.0f)   loop of single calls %8.0f (%.0f - %.0f)   ratio %.2f"
                     % ((nc, nk, found) + b + s + (s[0] / b[0],)))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
