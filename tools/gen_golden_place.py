"""(build container, needs the reference)  Records tests/golden/place_l1_scores.npz: pairs of BoW vectors and the double that the
reference's own DBoW2::L1Scoring::score returns for them.  The reference's ScoringObject.cpp and BowVector.cpp are compiled, as
they are, with the small main below into a temporary directory; only the recorded data is committed.  ScoringObject.cpp includes
TemplatedVocabulary.h, which needs OpenCV for code the scores never touch: its include guard is defined on the command line, so
the header is skipped, and ScoringObject.h and <cmath> (which it would have brought in) are included in its place.

    python tools/gen_golden_place.py [REFERENCE_ROOT]      (default: /root/reference)

The pairs: tf-idf-like positive weights that sum to 1 (integers over 2^20, stored as the integers), lengths 0, 1, 63, 64, 65 and
1500, disjoint, identical and partly overlapping word sets, both argument orders."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "BowVector.h"
#include "ScoringObject.h"
// stdin: int32 n_pairs, then per pair and side: int32 n, n x int32 word, n x double value.  stdout: n_pairs x double.
static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }
int main() {
    int32_t np = 0;
    if (!rd(&np, 4)) return 1;
    DBoW2::L1Scoring l1;
    for (int32_t i = 0; i < np; ++i) {
        DBoW2::BowVector v[2];
        for (int s = 0; s < 2; ++s) {
            int32_t n = 0;
            if (!rd(&n, 4)) return 1;
            std::vector<int32_t> w(n);
            std::vector<double> x(n);
            if (n && (!rd(w.data(), 4 * (size_t)n) || !rd(x.data(), 8 * (size_t)n))) return 1;
            for (int32_t k = 0; k < n; ++k) v[s].addWeight((DBoW2::WordId)w[k], x[k]);
        }
        const double r = l1.score(v[0], v[1]);
        fwrite(&r, 8, 1, stdout);
    }
    return 0;
}
"""


ONE = 1 << 20


def weights(rng, n):
    """n positive integers that sum to 2^20: the weights are these over 2^20, so they sum to exactly 1 and are stored as integers"""
    if n == 0:
        return np.zeros(0, np.int64)
    w = rng.gamma(2.0, 1.0, n) * rng.uniform(0.2, 9.0, n)       # tf * idf
    k = np.maximum(1, np.floor(w / w.sum() * (ONE - n)).astype(np.int64))
    k[np.argmax(k)] += ONE - k.sum()
    assert k.min() >= 1 and k.sum() == ONE
    return k


def pairs(seed=20):
    rng = np.random.default_rng(seed)
    out = []
    small = (0, 1, 63, 64, 65)
    # many pairs of the short lengths (they cost next to nothing), two overlaps per pair of wave-edge lengths, three long pairs
    combos = [(a, b, 25 if max(a, b) <= 1 else 6 if min(a, b) <= 1 else 2) for a in small for b in small]
    combos += [(1500, 0, 1), (1500, 65, 1), (1500, 1500, 1)]
    for na, nb, n_overlap in combos:
        for kind in (["overlap"] if na == 1500 else ["disjoint", "identical"]) + ["overlap"] * (n_overlap - (na == 1500)):
            if kind == "identical":
                if na != nb:
                    continue
                wa = np.sort(rng.choice(4 * max(na, 1), na, replace=False))
                va = weights(rng, na)
                out.append((wa, va, wa.copy(), va.copy()))
                out.append((wa, va, wa.copy(), weights(rng, na)))        # the same words, other weights
                continue
            if kind == "disjoint":
                wa = 2 * np.sort(rng.choice(4 * max(na, 1), na, replace=False))
                wb = 2 * np.sort(rng.choice(4 * max(nb, 1), nb, replace=False)) + 1
            else:
                span = int(max(na, nb, 1) * rng.choice([1.2, 2.0, 6.0]))
                wa = np.sort(rng.choice(span, na, replace=False))
                wb = np.sort(rng.choice(span, nb, replace=False))
            out.append((wa, weights(rng, na), wb, weights(rng, nb)))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    dbow = os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2")
    P = pairs()
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "main.cpp"), "w").write(MAIN)
        exe = os.path.join(tmp, "l1")
        subprocess.check_call(["g++", "-O0", "-std=c++11", "-ffp-contract=off", "-w", "-D__D_T_TEMPLATED_VOCABULARY__", "-include", "cmath", "-include",
                               os.path.join(dbow, "ScoringObject.h"), "-I" + dbow,
                               os.path.join(tmp, "main.cpp"), os.path.join(dbow, "ScoringObject.cpp"), os.path.join(dbow, "BowVector.cpp"),
                               "-o", exe])
        blob = struct.pack("<i", len(P))
        for wa, va, wb, vb in P:
            for w, v in ((wa, va), (wb, vb)):
                blob += struct.pack("<i", len(w)) + np.asarray(w, "<i4").tobytes() + (np.asarray(v, "<f8") / ONE).tobytes()
        raw = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
    score = np.frombuffer(raw, "<f8")
    assert len(score) == len(P)
    off = np.zeros((len(P), 3), np.int64)                       # pair i: side a = [off[i,0], off[i,1]), side b = [off[i,1], off[i,2])
    at = 0
    for i, (wa, va, wb, vb) in enumerate(P):
        off[i] = (at, at + len(wa), at + len(wa) + len(wb))
        at = off[i, 2]
    word = np.concatenate([np.concatenate([p[0], p[2]]) for p in P]).astype(np.int32)
    num = np.concatenate([np.concatenate([p[1], p[3]]) for p in P]).astype(np.int32)          # value = num / 2^20, exactly
    out = os.path.join(ROOT, "tests", "golden", "place_l1_scores.npz")
    np.savez_compressed(out, off=off, word=word, num=num, score=score)
    print("%d pairs, %d words, %d bytes -> %s" % (len(P), len(word), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
