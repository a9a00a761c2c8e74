"""CPU: OptimizerHip::OptimizeSim3 / OptimizeSim3Batch (include/qsp_optimizer_shim.h) and the drop-in's opt-in routing, compiled
against the stand-in map types of tests/shim_mock_sim3/ and a stub of qsp_sim3_optimize_batch that records what it is given and
answers with a fixed pattern.  A stand-alone program (sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_sim3")
_EXE = {}


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_sim3_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    cxx = ["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1", "-DQSP_SHIM_MOCK_SIM3=1"] + san + inc
    cc = ["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(cxx + ["-c", os.path.join(ROOT, "qsp_slam_amd", "orbslam", "Optimizer_hip.cc"), "-o", o("hip.o")])
    subprocess.check_call(cxx + ["-c", os.path.join(MOCK, "sim3_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(cc + ["-c", os.path.join(ROOT, "tests", "shim_mock", "stub_qsp.c"), "-o", o("stub.o")])
    subprocess.check_call(cc + ["-c", os.path.join(MOCK, "stub_sim3.c"), "-o", o("stub3.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("hip.o"), o("stub.o"), o("stub3.o")])
    _EXE["exe"] = o("caller")
    return _EXE["exe"]


def run(mode, **env_extra):
    with tempfile.TemporaryDirectory() as tmp:
        env = {k: v for k, v in os.environ.items() if not k.startswith("QSP_")}
        env.update(QSP_STUB_DUMP=os.path.join(tmp, "dump.txt"), QSP_G2O_LOG=os.path.join(tmp, "g2o.log"), **env_extra)
        r = subprocess.run([build(), mode], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        calls = []
        if os.path.exists(env["QSP_STUB_DUMP"]):
            for line in open(env["QSP_STUB_DUMP"]).read().splitlines():
                k, *v = line.split()
                if k == "call":
                    calls.append(dict(n_cand=int(v[0]), n_match=int(v[1]), th2=float(v[2]), fix=int(v[3])))
                else:
                    calls[-1][k] = np.array(v, np.float64)
        log = open(env["QSP_G2O_LOG"]).read().splitlines() if os.path.exists(env["QSP_G2O_LOG"]) else []
    res = {}
    for line in r.stdout.splitlines():
        if "|" in line:
            head, flags, s = line.split("|")
            res[head.split()[0]] = dict(n=int(head.split()[1]), kept=[int(x) for x in flags.split()], sim3=np.array(s.split(), np.float64))
        else:
            t = line.split()
            res.update({t[i]: int(t[i + 1]) for i in range(0, len(t), 2)})
    return res, calls, log, r.stderr


# ---- the caller's procedural scene, restated ---------------------------------------------------------------------------------
f32 = np.float32
N = 20


def kf(k):
    a = 0.1 * k
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).astype(f32)
    t = np.array([f32(0.1) * f32(r + 1) * f32(k) for r in range(3)], f32)
    K = [f32(500) + f32(k), f32(510) + f32(k), f32(320) + f32(0.5) * f32(k), f32(240) + f32(0.25) * f32(k)]
    keys = lambda j: (f32(100) * f32(k) + f32(7) * f32(j) + f32(0.25), f32(50) + f32(5) * f32(j) + f32(0.5) * f32(k), j % 4)
    sig = [f32(1) / f32(1 << o) for o in range(4)]
    return dict(R=R, t=t, K=np.array(K, np.float64), key=keys, sig=sig)


def to_camera(F, X):
    """the shim's reading of cv::Mat R * X + t in float32: row products summed in double, rounded to float, t added in float"""
    rx = (F["R"].astype(np.float64) * X.astype(np.float64)).cumsum(axis=1)[:, -1].astype(f32)
    return (rx + F["t"]).astype(f32).astype(np.float64)


def expected(c):
    """what candidate c (0: key frame 2, 1: key frame 3) must flatten to: kept slots, P1 P2 o1 o2 i1 i2"""
    F1, F2 = kf(1), kf(2 + c)
    slots = [i for i in range(N) if i not in (2, 3, 5, 7, 9) and not (c == 1 and i >= 10)]
    P1, P2, o1, o2, i1, i2 = [], [], [], [], [], []
    for i in slots:
        P1.append(to_camera(F1, np.array([f32(0.1) * f32(i) - f32(0.5), f32(0.05) * f32(i), f32(2) + f32(0.3) * f32(i)], f32)))
        P2.append(to_camera(F2, np.array([f32(0.1) * f32(i) - f32(0.4), f32(0.05) * f32(i) + f32(0.1) * f32(c),
                                          f32(2.5) + f32(0.3) * f32(i)], f32)))
        u, v, o = F1["key"](i)
        o1.append([u, v]); i1.append(F1["sig"][o])
        u, v, o = F2["key"]((i * 3 + c) % 25)
        o2.append([u, v]); i2.append(F2["sig"][o])
    cat = lambda a: np.array(a, np.float64).reshape(-1)
    return slots, dict(P1=cat(P1), P2=cat(P2), o1=cat(o1), o2=cat(o2), i1=cat(i1), i2=cat(i2), K1=F1["K"], K2=F2["K"])


S2 = np.array([1, 2, 3, 0.1, -0.2, 0.3, 0.9, 1.25])
S3 = np.array([-1, 0.5, 4, -0.3, 0.2, 0.1, 0.8, 0.75])


def kept_after(slots, n_total=N, c=0):
    """the stub drops position e % 3 == 1 of a candidate: those slots become NULL; the others keep their pointers"""
    start = [0 if (i == 2 or (c == 1 and i >= 10)) else 1 for i in range(n_total)]
    for e, i in enumerate(slots):
        if e % 3 == 1:
            start[i] = 0
    return start


def test_flattening_filters_order_and_widening():
    res, calls, _, _ = run("single")
    assert len(calls) == 2 and [c["n_cand"] for c in calls] == [1, 1]
    assert (calls[0]["th2"], calls[0]["fix"]) == (10.0, 1) and calls[1]["fix"] == 0
    for c, call, S in ((0, calls[0], S2), (1, calls[1], S3)):
        slots, e = expected(c)
        assert call["n_match"] == len(slots) and list(call["off"]) == [0, len(slots)]
        for k, v in e.items():
            assert np.array_equal(call[k], v), (c, k)                      # float -> double: the float values, bit for bit
        assert np.array_equal(call["S"], S)


def test_write_back_on_the_full_and_on_the_early_return_path():
    res, _, _, _ = run("single")
    s0, s1 = expected(0)[0], expected(1)[0]
    assert res["status"] == 0
    assert res["full"]["n"] == sum(1 for e in range(len(s0)) if e % 3 != 1) and res["full"]["kept"] == kept_after(s0)
    assert np.array_equal(res["full"]["sim3"], S2 + np.array([0.5, 0, 0, 0, 0, 0, 0, 1.25]))          # g2oS12 written
    assert res["early"]["n"] == 0 and res["early"]["kept"] == kept_after(s1, c=1)                      # NULLs written all the same
    assert np.array_equal(res["early"]["sim3"], S3)                                                    # g2oS12 not written


def test_batch_form_is_one_call_with_offsets():
    res, calls, _, _ = run("batch")
    assert len(calls) == 1 and calls[0]["n_cand"] == 2
    (s0, e0), (s1, e1) = expected(0), expected(1)
    assert list(calls[0]["off"]) == [0, len(s0), len(s0) + len(s1)]
    for k in ("P1", "P2", "o1", "o2", "i1", "i2"):
        assert np.array_equal(calls[0][k], np.concatenate([e0[k], e1[k]])), k
    assert np.array_equal(calls[0]["K2"], np.concatenate([e0["K2"], e1["K2"]]))
    assert np.array_equal(calls[0]["S"], np.concatenate([S2, S3]))
    single = run("single")[0]
    for k in ("full", "early"):
        assert res[k]["n"] == single[k]["n"] and res[k]["kept"] == single[k]["kept"] and np.array_equal(res[k]["sim3"], single[k]["sim3"])


def test_default_dropin_still_reaches_g2o():
    res, calls, log, err = run("dropin")
    assert calls == [] and [l.split()[0] for l in log] == ["g2o:OptimizeSim3"]
    assert res["dropin"]["n"] == 17 and res["dropin"]["sim3"][7] == 42.0 and res["failures"] == 0


def test_opt_in_reaches_the_library():
    res, calls, log, err = run("dropin", QSP_SHIM_SIM3_HIP="1")
    assert len(calls) == 1 and log == [] and calls[0]["fix"] == 1 and calls[0]["th2"] == 10.0
    assert res["dropin"]["kept"] == kept_after(expected(0)[0]) and res["dropin"]["sim3"][7] == 2.5 and res["failures"] == 0


def test_failure_row():
    """a failed call: matches and g2oS12 untouched, 0 returned, the counters move, g2o only where the deployment opted in"""
    res, calls, log, err = run("dropin", QSP_SHIM_SIM3_HIP="1", QSP_STUB_FAIL="sim3")
    assert res["dropin"]["n"] == 0 and res["dropin"]["kept"] == [0 if i == 2 else 1 for i in range(N)]
    assert np.array_equal(res["dropin"]["sim3"], S2) and log == []
    assert res["failures"] == 1 and res["fallbacks"] == 0 and "the map is left untouched" in err
    res, calls, log, err = run("dropin", QSP_SHIM_SIM3_HIP="1", QSP_STUB_FAIL="sim3", QSP_SHIM_ALLOW_G2O_FALLBACK="1")
    assert [l.split()[0] for l in log] == ["g2o:OptimizeSim3"] and res["dropin"]["n"] == 17
    assert res["failures"] == 1 and res["fallbacks"] == 1 and "falls back" in err
