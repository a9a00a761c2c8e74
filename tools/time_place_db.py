"""Times the resident place-recognition database (qsp_place_db) on the GPU: one LOOP and one RELOC detection (query + accumulate)
against 500 and 5000 listed key frames of about 1500 words each out of a vocabulary of 10^5 ids, with a planted group of key
frames similar to the query so that the score, order and covisibility stages have work.  Median and min-max of 30 calls after
warm-up, host wall clock around the whole call through the Python binding; the cost of one put; the device bytes the handle
holds.  The kernels' own times come from a child run of this script under `rocprofv3 --kernel-trace --stats` (skipped, and said
so, where rocprofv3 is missing; a child that fails or hangs is killed with its process group and ends the tool with an error, and
the children run only after this process's own GPU work is done).  The reference's KeyFrameDatabase needs OpenCV and DBoW2 and was not built or timed: no CPU
comparison.

    python tools/time_place_db.py [--out FILE] [--commit TEXT]   (default: profiles/place_db.txt)"""
import csv
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOCAB, N_WORDS, N_PLANTED = 100000, 1500, 40
KERNELS = ("k_place_common", "k_place_score", "k_place_order", "k_place_acc", "k_place_mark")


def bow(rng, words):
    v = rng.gamma(2.0, 1.0, len(words)) * rng.uniform(0.2, 9.0, len(words))
    return np.sort(words).astype(np.int32), v / v.sum()


def scene(n_kf, seed=3):
    """the query, n_kf key frames (the first N_PLANTED share about 0.85 - 1.0 of the query's words, the rest are random), a neighbour
    table of 10 ids each, the connected ids and the refs of a LOOP query"""
    rng = np.random.default_rng(seed)
    q = rng.choice(VOCAB, N_WORDS, replace=False)
    kfs = []
    for i in range(n_kf):
        if i < N_PLANTED:
            keep = q[rng.uniform(size=N_WORDS) < rng.uniform(0.85, 1.0)]
            rest = np.setdiff1d(rng.choice(VOCAB, 2 * N_WORDS, replace=False), q)[:N_WORDS - len(keep)]
            kfs.append(bow(rng, np.concatenate([keep, rest])))
        else:
            kfs.append(bow(rng, rng.choice(VOCAB, N_WORDS, replace=False)))
    order = rng.permutation(n_kf)                              # the planted ones are spread over the list
    nb = {int(i): [int(x) for x in rng.choice(N_PLANTED + 20, 10, replace=False)] for i in range(n_kf)}
    return bow(rng, q), kfs, order, nb, [int(x) for x in range(N_PLANTED, N_PLANTED + 15)], [int(x) for x in range(N_PLANTED + 15, N_PLANTED + 30)]


def fill(n_kf):
    from qsp_slam_amd.ba import PlaceDatabase
    q, kfs, order, nb, conn, refs = scene(n_kf)
    db = PlaceDatabase()
    t_put = []
    for i in order:
        t = time.perf_counter()
        db.put(int(i), *kfs[i])
        t_put.append((time.perf_counter() - t) * 1e6)
    return db, q, nb, conn, refs, t_put


def kernel_times(n_kf):
    """{kernel: (mean us, calls)} from a child run under rocprofv3; None only where rocprofv3 is missing or left no statistics after
    a clean exit.  A child that fails or runs out of time ends this tool at once, with its whole process group killed: nothing more
    is started on a card after something went wrong on it."""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return None
    tmp = tempfile.mkdtemp(prefix="qsp_place_prof_")
    try:
        child = subprocess.Popen([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                                  os.path.abspath(__file__), "--child", str(n_kf)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                                 start_new_session=True)
        try:
            rc = child.wait(timeout=300)
        except subprocess.TimeoutExpired:
            rc = None
        if rc != 0:
            try:
                os.killpg(child.pid, signal.SIGKILL)             # rocprofv3 AND the python under it
            except ProcessLookupError:
                pass
            child.wait()
            sys.exit("time_place_db: the profiled child run at %d key frames %s; nothing further is run on the GPU"
                     % (n_kf, "ran past 300 s and was killed" if rc is None else "ended with exit status %d" % rc))
        files = glob.glob(tmp + "/**/*kernel_stats.csv", recursive=True)
        if not files:
            return None
        out = {}
        for r in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if k in r["Name"]:
                    out[k] = (float(r["AverageNs"]) / 1e3, int(r["Calls"]))
        return out or None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    argv, opt = sys.argv[1:], {}
    if argv and argv[0] == "--child":                   # the profiled run: 10 detections of each mode, nothing else
        db, q, nb, conn, refs, _ = fill(int(argv[1]))
        for _ in range(10):
            db.detect_loop_candidates(q[0], q[1], nb, excluded=conn, ref_ids=refs)
            db.detect_relocalization_candidates(q[0], q[1], nb)
        db.close()
        return
    for name in ("--out", "--commit"):                  # --commit TEXT: where no git metadata travels with the tree
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    out = opt.get("--out", os.path.join(ROOT, "profiles", "place_db.txt"))
    commit = opt.get("--commit")
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown (no git metadata here)"
    lines = ["qsp_place_db: one detection = qsp_place_db_query + qsp_place_db_accumulate; key frames of %d words out of a vocabulary of %d ids, "
             "%d of them planted near the query; LOOP with 15 connected key frames excluded and DetectLoop's minimum score over 15 refs"
             % (N_WORDS, VOCAB, N_PLANTED),
             "host wall clock per call in microseconds through the Python binding, 30 calls after 3 warm-up calls: median (min - max); "
             "measured with the library sources of commit %s" % commit,
             "the reference's KeyFrameDatabase (CPU, OpenCV + DBoW2) was not built or measured here: no CPU comparison, no speed-up claimed", ""]

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(30):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return np.median(ts), min(ts), max(ts)

    blocks = []
    for n_kf in (500, 5000):                            # this process's own GPU work first ...
        db, q, nb, conn, refs, t_put = fill(n_kf)
        r = db.detect_loop_candidates(q[0], q[1], nb, excluded=conn, ref_ids=refs)
        s = db.detect_relocalization_candidates(q[0], q[1], nb)
        blk = ["%d listed key frames: device bytes held %d; one put (host wall clock, us) median %.0f (%.0f - %.0f)"
               % ((n_kf, db.size()["device_bytes"], np.median(t_put), min(t_put), max(t_put)))]
        for label, res, fn, qfn in (
                ("LOOP ", r, lambda: db.detect_loop_candidates(q[0], q[1], nb, excluded=conn, ref_ids=refs),
                 lambda: db.query(db.LOOP, q[0], q[1], excluded=conn, ref_ids=refs, tap=False)),
                ("RELOC", s, lambda: db.detect_relocalization_candidates(q[0], q[1], nb), lambda: db.query(db.RELOC, q[0], q[1], tap=False))):
            blk.append("  %s  sharing %4d  max common %4d  scored and kept %3d  candidates %2d:  detection %7.0f (%.0f - %.0f)   of which query alone %7.0f (%.0f - %.0f)"
                       % ((label, res["n_sharing"], res["max_common"], len(res["match_id"]), len(res["cand_id"])) + clock(fn) + clock(qfn)))
        db.close()
        blocks.append((n_kf, blk))
    for n_kf, blk in blocks:                            # ... then the profiled children, one after the other; a failed one ends the tool
        kt = kernel_times(n_kf)
        if kt is None:
            blk.append("  kernel times not measured (rocprofv3 is missing or left no kernel statistics)")
        else:
            blk.append("  the kernels' own times (rocprofv3 --kernel-trace --stats over 10 detections of each mode, mean per launch in us):  "
                       + "   ".join("%s %.1f (%d launches)" % (k, kt[k][0], kt[k][1]) for k in KERNELS if k in kt))
        lines += blk
    txt = "\n".join(lines) + "\n"
    print(txt)
    if out:
        open(out, "w").write(txt)


if __name__ == "__main__":
    main()
