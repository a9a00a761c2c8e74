"""Batched mesh extraction against a loop of single calls, same process, same codes, results fetched to the host in both:
ms per mesh of MeshExtractor.extract_meshes_from_codes and of a loop over extract_mesh_from_code at 32^3 and 64^3 for batches
of 1, 8 and 64 codes -- median [min .. max] over REPS alternating repetitions after warm-up -- and the mesh counts of both, which
must agree.   python tools/mesh_batch.py [precision]"""
import contextlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from qsp_slam_amd import DeepSdfDecoder
from qsp_slam_amd.reconstruct.optimizer import MeshExtractor
REPS, WARM = 12, 3
prec = sys.argv[1] if len(sys.argv) > 1 else "f32"
dec = DeepSdfDecoder.from_npz(os.path.join(ROOT, "tests", "golden", "decoder_8x512.npz"))
dec.set_precision(prec)


def stats(ts, n):
    ms = 1e3 * np.asarray(ts) / n
    return "%7.3f [%7.3f .. %7.3f]" % (np.median(ms), ms.min(), ms.max())


for dim in (32, 64):
    me = MeshExtractor(dec, 64, dim)
    for n in (1, 8, 64):
        codes = (0.05 * np.random.default_rng(n).standard_normal((n, 64))).astype(np.float32)
        tb, tl = [], []
        with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):      # (the mirror prints the reference's "Extract mesh takes ..." line)
            for rep in range(WARM + REPS):
                t0 = time.perf_counter()
                batch = me.extract_meshes_from_codes(codes)
                t1 = time.perf_counter()
                loop = [me.extract_mesh_from_code(c) for c in codes]
                t2 = time.perf_counter()
                if rep >= WARM:
                    tb.append(t1 - t0)
                    tl.append(t2 - t1)
        cb = (sum(len(m.vertices) for m in batch), sum(len(m.faces) for m in batch))
        cl = (sum(len(m.vertices) for m in loop), sum(len(m.faces) for m in loop))
        assert cb == cl and all(np.array_equal(a.faces, b.faces) for a, b in zip(batch, loop)), (cb, cl)
        print("%s %3d^3 batch %2d: batched %s ms per mesh | loop of single calls %s ms per mesh | %d vertices, %d faces in both"
              % (prec, dim, n, stats(tb, n), stats(tl, n), cb[0], cb[1]))
