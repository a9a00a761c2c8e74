"""Mesh extraction over a decoder group against one batched call per class, same process, same codes, results fetched to the
host in both: three classes (decoder_8x512, the same with use_tanh, the same with perturbed weights) with 1, 8 and 21 codes per
class at 32^3 and 64^3; ms per mesh of ONE MeshExtractorGroup.extract_meshes_from_codes call (classes interleaved, and the same
items sorted by class: what staging a decoder's constants again at every volume boundary costs) and of the three per-class
MeshExtractor.extract_meshes_from_codes calls it replaces -- median [min .. max] over REPS alternating repetitions after warm-up,
all warm -- and the ratios of the medians.  The meshes of both must agree.   python tools/mesh_group.py [precision]"""
import contextlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from qsp_slam_amd import DeepSdfDecoder
from qsp_slam_amd.reconstruct.optimizer import MeshExtractor, MeshExtractorGroup
REPS, WARM = 12, 3
prec = sys.argv[1] if len(sys.argv) > 1 else "f32"
path = os.path.join(ROOT, "tests", "golden", "decoder_8x512.npz")
z = np.load(path, allow_pickle=False)
rng = np.random.default_rng(5)
state = {k: (z[k] * (1.0 + 0.02 * rng.standard_normal(z[k].shape))).astype(np.float32) for k in z.files if k != "meta"}
decs = [DeepSdfDecoder.from_npz(path), DeepSdfDecoder.from_npz(path), DeepSdfDecoder.from_state_dict(state)]
decs[1].set_use_tanh(True)
for d in decs:
    d.set_precision(prec)


def stats(ts, n):
    ms = 1e3 * np.asarray(ts) / n
    return "%7.3f [%7.3f .. %7.3f]" % (np.median(ms), ms.min(), ms.max())


for dim in (32, 64):
    ext = {c: MeshExtractor(d, 64, dim) for c, d in enumerate(decs)}
    mg = MeshExtractorGroup(ext)
    for per in (1, 8, 21):
        n = 3 * per
        codes = (0.05 * np.random.default_rng(n).standard_normal((n, 64))).astype(np.float32)
        cls = [i % 3 for i in range(n)]
        order = sorted(range(n), key=lambda i: cls[i])
        of_class = {c: [i for i in range(n) if cls[i] == c] for c in ext}
        tg, ts, tc = [], [], []
        with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):      # (the mirror prints the reference's "Extract ... takes" line)
            for rep in range(WARM + REPS):
                t0 = time.perf_counter()
                mixed = mg.extract_meshes_from_codes(codes, cls)
                t1 = time.perf_counter()
                by_class = mg.extract_meshes_from_codes(codes[order], [cls[i] for i in order])
                t2 = time.perf_counter()
                each = {c: ext[c].extract_meshes_from_codes(codes[of_class[c]]) for c in ext}
                t3 = time.perf_counter()
                if rep >= WARM:
                    tg.append(t1 - t0)
                    ts.append(t2 - t1)
                    tc.append(t3 - t2)
        loop = [None] * n
        for c in ext:
            for i, m in zip(of_class[c], each[c]):
                loop[i] = m
        assert all(a is not None and np.array_equal(a.faces, b.faces) and np.array_equal(a.vertices, b.vertices) for a, b in zip(mixed, loop))
        assert all(np.array_equal(by_class[k].faces, loop[i].faces) for k, i in enumerate(order))
        g, s, c3 = (np.median(t) for t in (tg, ts, tc))
        print("%s %3d^3 3 x %2d codes: one group call %s ms per mesh | sorted by class %s | three per-class calls %s | "
              "group / per-class %.3f, sorted / interleaved %.3f | %d vertices, %d faces in both"
              % (prec, dim, per, stats(tg, n), stats(ts, n), stats(tc, n), g / c3, s / g,
                 sum(len(m.vertices) for m in mixed), sum(len(m.faces) for m in mixed)))
    mg.close()
