"""CPU: Sim3SolverHip::FindBatch (include/qsp_optimizer_shim.h), compiled against the stand-in map types of tests/shim_mock_ransac/
and a stub of qsp_sim3_ransac_batch that records what it is given and answers with a fixed pattern.  A stand-alone program
(sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_ransac")
_EXE = {}


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_ransac_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc
                          + ["-c", os.path.join(MOCK, "ransac_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_ransac.c"),
                                                              "-o", o("stub.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("stub.o")])
    _EXE["exe"] = o("caller")
    return _EXE["exe"]


def run(mode="", **env_extra):
    with tempfile.TemporaryDirectory() as tmp:
        env = {k: v for k, v in os.environ.items() if not k.startswith("QSP_")}
        env.update(QSP_STUB_DUMP=os.path.join(tmp, "dump.txt"), **env_extra)
        r = subprocess.run([build(), mode], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        calls = []
        if os.path.exists(env["QSP_STUB_DUMP"]):
            for line in open(env["QSP_STUB_DUMP"]).read().splitlines():
                k, *v = line.split()
                if k == "call":
                    calls.append(dict(zip(("n_cand", "n_match", "n_trip", "min_inliers", "fix", "tap"), map(int, v))))
                else:
                    calls[-1][k] = np.array(v, np.int64 if k in ("off", "its", "toff", "tri") else np.float32)
    res = dict(cand=[])
    for line in r.stdout.splitlines():
        if "|" in line:
            head, R, t, flags = line.split("|")
            h = head.split()
            res["cand"].append(dict(N=int(h[2]), its=int(h[3]), first=int(h[4]), n_in=int(h[5]), s=float(h[6]),
                                    R=np.array(R.split(), np.float32), t=np.array(t.split(), np.float32),
                                    flags=[int(x) for x in flags.split()]))
        else:
            k, *v = line.split()
            res[k] = [int(x) for x in v]
    return res, calls, r.stderr


# ---- the caller's procedural scene, restated ---------------------------------------------------------------------------------
f32 = np.float32
N_SLOTS, N_KEYS = 30, 40
SIG, _s = [], f32(1)                                         # mvLevelSigma2 as the caller fills it
for _o in range(4):
    SIG.append(f32(_s * _s))
    _s = f32(_s * f32(1.2))


def kf(k):
    a = 0.1 * k
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).astype(f32)
    t = np.array([f32(0.1) * f32(r + 1) * f32(k) for r in range(3)], f32)
    K = np.array([f32(500) + f32(k), f32(510) + f32(k), f32(320) + f32(0.5) * f32(k), f32(240) + f32(0.25) * f32(k)], f32)
    return dict(R=R, t=t, K=K)


def to_camera(F, X):
    """cv::Mat R * X + t in float32: the row product summed in double and rounded to float, t added in float"""
    rx = (F["R"].astype(np.float64) * X.astype(np.float64)).cumsum(axis=1)[:, -1].astype(f32)
    return (rx + F["t"]).astype(f32)


def slots_of(c):
    """the slots the constructor keeps for candidate c: not the null match (2), null / unobserved / bad pMP1 (3, 4, 5), bad or
    unobserved pMP2 (7, 9), nor what the candidate's match vector leaves empty"""
    return [i for i in range(N_SLOTS) if i not in (2, 3, 4, 5, 7, 9) and not (c == 2 and i >= 15) and not (c == 4 and i >= 26)]


def expected(c):
    F1, F2 = kf(1), kf(2 + c)
    X1, X2, s1, s2 = [], [], [], []
    for i in slots_of(c):
        X1.append(to_camera(F1, np.array([f32(0.1) * f32(i) - f32(0.5), f32(0.05) * f32(i), f32(2) + f32(0.3) * f32(i)], f32)))
        X2.append(to_camera(F2, np.array([f32(0.1) * f32(i) - f32(0.4), f32(0.05) * f32(i) + f32(0.1) * f32(c),
                                          f32(2.5) + f32(0.3) * f32(i)], f32)))
        s1.append(SIG[((i * 2) % N_KEYS) % 4])
        s2.append(SIG[((i * 3 + c) % N_KEYS) % 4])
    cat = lambda a: np.array(a, f32).reshape(-1)
    return dict(X1=cat(X1), X2=cat(X2), s1=cat(s1), s2=cat(s2), K1=F1["K"], K2=F2["K"])


def iterations(n):
    from tests.sim3_ransac_oracle import iterations as it
    return it(n) or 0


def expected_triples():
    """the caller's draw(lo, hi) = lo + (17 k + 3) % (hi - lo + 1) through draw-and-swap-with-back, candidate after candidate"""
    k, tri, his = 0, [], []
    for c in range(5):
        n = len(slots_of(c))
        for _ in range(iterations(n)):
            avail = list(range(n))
            for _i in range(3):
                his.append(len(avail) - 1)
                r = (17 * k + 3) % len(avail)
                k += 1
                tri.append(avail[r])
                avail[r] = avail[-1]
                avail.pop()
    return tri, his


FIRST = [6, 3, 0, 5, 1]                                      # the stub's pattern under these iteration counts


def test_constructor_skips_and_flattening():
    res, calls, _ = run()
    assert res["status"] == [0] and len(calls) == 1
    call = calls[0]
    n = [len(slots_of(c)) for c in range(5)]
    assert n == [24, 24, 9, 24, 20]
    assert (call["n_cand"], call["min_inliers"], call["fix"], call["tap"]) == (5, 20, 0, 0)
    assert list(call["off"]) == [0] + list(np.cumsum(n)) and call["n_match"] == sum(n)
    e = [expected(c) for c in range(5)]
    for key in ("X1", "X2", "s1", "s2", "K2"):
        assert np.array_equal(call[key], np.concatenate([x[key] for x in e])), key
    assert np.array_equal(call["K1"], np.tile(e[0]["K1"], 5))
    assert run("fix")[1][0]["fix"] == 1


def test_iteration_counts_and_triples():
    res, calls, _ = run()
    its = [iterations(len(slots_of(c))) for c in range(5)]
    assert its == [6, 6, 0, 6, 1]                            # 24 matches: ceil(log .01 / log(1 - (20/24)^3)) = 6; 9: none; 20: 1
    assert list(calls[0]["its"]) == its and list(calls[0]["toff"]) == [0] + list(np.cumsum(its))
    assert [c["its"] for c in res["cand"]] == its and [c["N"] for c in res["cand"]] == [24, 24, 9, 24, 20]
    tri, his = expected_triples()
    assert list(calls[0]["tri"]) == tri and res["his"] == his and res["lo_bad"] == [0]
    assert res["small"] == [0, 0, 1, 35]                     # N < 3: nothing to draw; N == minInliers: 1; eps = 2/4: ceil(34.49) = 35
    t = np.array(tri).reshape(-1, 3)
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()


def test_results_are_scattered_through_the_kept_slots():
    res, _, _ = run()
    for c, r in enumerate(res["cand"]):
        assert r["first"] == FIRST[c] and len(r["flags"]) == N_SLOTS
        slots = slots_of(c)
        want = [0] * N_SLOTS
        if FIRST[c]:
            for e, i in enumerate(slots):
                want[i] = int(e % 2 == 0)
            assert np.array_equal(r["R"], np.array([c + 0.25 * i for i in range(9)], f32))
            assert np.array_equal(r["t"], np.array([10 * c + i for i in range(3)], f32)) and r["s"] == 1 + c
        else:
            assert not r["R"].any() and not r["t"].any() and r["s"] == 0
        assert r["flags"] == want and r["n_in"] == sum(want)


def test_round_robin_order():
    """five iterations per visit: candidates 1, 3, 4 succeed in the first pass (iterations 3, 5, 1) in index order, candidate 0 in
    the second (iteration 6), candidate 2 never"""
    res, _, _ = run()
    assert res["order"] == [1, 3, 4, 0]
    assert res["order"] == sorted([c for c in range(5) if FIRST[c]], key=lambda c: ((FIRST[c] + 4) // 5, c))


def test_a_failed_call_leaves_the_outputs_untouched():
    res, calls, err = run("prefilled", QSP_STUB_FAIL="ransac")
    assert res["status"] == [3] and calls == []
    assert res["order"] == [5] and len(res["cand"]) == 1 and res["cand"][0]["first"] == 77
    assert "qsp_sim3_ransac_batch failed" in err
    res, _, _ = run("prefilled")                            # and a successful one replaces them
    assert res["status"] == [0] and res["order"] == [1, 3, 4, 0] and len(res["cand"]) == 5
