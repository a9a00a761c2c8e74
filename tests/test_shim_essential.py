"""CPU: OptimizerHip::OptimizeEssentialGraph (include/qsp_optimizer_shim.h) and the drop-in's opt-in routing, compiled against the
stand-in map types of tests/shim_mock_essential/ and a stub of qsp_essential_graph_optimize that records what it is given and
answers with a fixed pattern.  A stand-alone program (sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

import numpy as np

from tests.sim3_oracle import s_inv, s_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_essential")
_EXE = {}


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_essential_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    cxx = ["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1", "-DQSP_SHIM_MOCK_SIM3=1", "-DQSP_SHIM_MOCK_ESSENTIAL=1"] + san + inc
    cc = ["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(cxx + ["-c", os.path.join(ROOT, "qsp_slam_amd", "orbslam", "Optimizer_hip.cc"), "-o", o("hip.o")])
    subprocess.check_call(cxx + ["-c", os.path.join(MOCK, "essential_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(cc + ["-c", os.path.join(ROOT, "tests", "shim_mock", "stub_qsp.c"), "-o", o("stub.o")])
    subprocess.check_call(cc + ["-c", os.path.join(ROOT, "tests", "shim_mock_sim3", "stub_sim3.c"), "-o", o("stub3.o")])
    subprocess.check_call(cc + ["-c", os.path.join(MOCK, "stub_essential.c"), "-o", o("stube.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("hip.o"), o("stub.o"), o("stub3.o"), o("stube.o")])
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
                    calls.append(dict(n_kf=int(v[0]), n_edge=int(v[1]), n_pt=int(v[2]), fix=int(v[3]), n_iter=int(v[4]), lam=float(v[5])))
                else:
                    calls[-1][k] = np.array(v, np.float64)
        log = open(env["QSP_G2O_LOG"]).read().splitlines() if os.path.exists(env["QSP_G2O_LOG"]) else []
    res = dict(kf={}, mp={})
    for line in r.stdout.splitlines():
        if "|" in line:
            head, vals = line.split("|")
            kind, i, n = head.split()
            res[kind][int(i)] = dict(n=int(n), v=np.array(vals.split(), np.float32).astype(np.float64))     # (%.9g round-trips a float)
        else:
            t = line.split()
            res.update({t[i]: int(t[i + 1]) for i in range(0, len(t), 2)})
    return res, calls, log, r.stderr


# ---- the caller's procedural scene, restated ---------------------------------------------------------------------------------
f32 = np.float32
IDS = [0, 1, 2, 3, 4, 5, 7]                                  # vertices in hessian order: key frame 6 is bad
IDX = {k: i for i, k in enumerate(IDS)}
CORR = {7: np.array([1, 2, 3, 0.1, -0.2, 0.3, 0.9, 1.25]), 5: np.array([-1, 0.5, 4, -0.3, 0.2, 0.1, 0.8, 0.75])}
NONC = {7: np.array([0.5, -2, 1, 0.2, 0.1, -0.3, 0.7, 1.0]), 5: np.array([2, 1, -1, 0.3, -0.1, 0.2, 0.6, 1.0])}
# the reference's insertion order.  Loop connections (map and sets ordered by pointer = id here): 5 -> {1: weight 30, dropped; 3},
# 7 -> {0: weight 50, dropped; 1: weight 20, kept as the current -> loop key frame pair; 2}.  Then per key frame in map order
# 3 0 5 1 7 2 6 4: the parent, loop edges to lower ids, covisibles of weight >= 100 without the parent, children, loop edges,
# bad key frames, higher ids, NULL entries and pairs already inserted as loop connections.
EDGES = [(5, 3), (7, 1), (7, 2),
         (3, 2), (3, 1), (3, 0),                             # 3: covisibles 1, [5 higher], [2 parent], [NULL], 0, [4: weight 90]
         (5, 4), (5, 2),                                     # 5: [3 inserted], [4 parent], 2
         (1, 4),
         (7, 5), (7, 3),                                     # 7: [2 inserted], 3, [5 parent]
         (2, 1),                                             # 2: loop edge 4 has the higher id
         (4, 3), (4, 2), (4, 0)]                             # 4: loop edge 2; covisibles [3 parent], [2 loop edge], [1 child], 0, [6 bad]
N_LOOP = 3


def tcw(k):
    a = 0.1 * k
    T = np.eye(4, dtype=f32)
    T[:2, :2] = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).astype(f32)
    T[:3, 3] = [f32(0.1) * f32(r + 1) * f32(k) for r in range(3)]
    return T


def rot_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_vertices_edges_and_measurements():
    res, calls, log, _ = run("member")
    assert res["status"] == 0 and len(calls) == 1 and log == []
    c = calls[0]
    assert (c["n_kf"], c["n_edge"], c["fix"], c["n_iter"], c["lam"]) == (7, len(EDGES), 1, 20, 1e-16)
    assert list(c["fixed"]) == [1 if k == 1 else 0 for k in IDS]
    S = c["S"].reshape(7, 8)
    for k in IDS:
        if k in CORR:
            assert np.array_equal(S[IDX[k]], CORR[k]), k                   # CorrectedSim3 where there is one
        else:
            T = tcw(k).astype(np.float64)
            assert S[IDX[k], 7] == 1.0 and np.array_equal(S[IDX[k], :3], T[:3, 3])
            assert np.abs(rot_of(S[IDX[k], 3:7]) - T[:3, :3]).max() < 1e-7 and abs(np.linalg.norm(S[IDX[k], 3:7]) - 1) < 1e-15
    assert [(int(a), int(b)) for a, b in zip(c["v0"], c["v1"])] == [(IDX[i], IDX[j]) for i, j in EDGES]
    Z = c["meas"].reshape(-1, 8)
    for e, (i, j) in enumerate(EDGES):
        if e < N_LOOP:                                                         # between the vertices' estimates (vScw)
            Si, Sj = S[IDX[i]], S[IDX[j]]
        else:                                                                  # NonCorrectedSim3 where present
            Si, Sj = NONC.get(i, S[IDX[i]]), NONC.get(j, S[IDX[j]])
        assert np.abs(Z[e] - s_mul(Sj, s_inv(Si))).max() < 1e-15, (e, i, j)
    assert any(i in NONC or j in NONC for i, j in EDGES[N_LOOP:])


def test_points_sent_and_write_back():
    res, calls, _, _ = run("member")
    c = calls[0]
    pos = lambda i: np.array([f32(0.25) * f32(i) + f32(0.5) * f32(r) for r in range(3)], np.float64)
    # point 1 is bad, point 3's reference key frame (6) is bad; point 2 was corrected by the current key frame: mnCorrectedReference
    assert c["n_pt"] == 3 and list(c["ref"]) == [IDX[3], IDX[5], IDX[1]]
    assert np.array_equal(c["P"], np.concatenate([pos(0), pos(2), pos(4)]))
    for i, r in ((0, IDX[3]), (2, IDX[5]), (4, IDX[1])):
        want = pos(i)
        want[0] += 0.5 * (r + 1)
        assert res["mp"][i]["n"] == 1 and np.array_equal(res["mp"][i]["v"], want.astype(f32).astype(np.float64)), i
    for i in (1, 3):
        assert res["mp"][i]["n"] == 0 and np.array_equal(res["mp"][i]["v"], pos(i)), i
    S = c["S"].reshape(7, 8)
    for k in range(8):
        T = res["kf"][k]["v"].reshape(4, 4)
        if k == 6:                                                             # bad: untouched
            assert res["kf"][k]["n"] == 0 and np.array_equal(T, tcw(k).astype(np.float64))
            continue
        assert res["kf"][k]["n"] == 1
        s8 = S[IDX[k]].copy()
        if k != 1:                                                             # the stub: t + (1, 2, 3), scale 2
            s8[:3] += [1, 2, 3]
            s8[7] = 2.0
        want = np.eye(4)
        want[:3, :3] = rot_of(s8[3:7])
        want[:3, 3] = s8[:3] * (1. / s8[7])                                    # [R t/s; 0 1]
        assert np.array_equal(T[:, 3], want.astype(f32).astype(np.float64)[:, 3]), k           # t/s, the float of the double
        assert np.abs(T[:3, :3] - want[:3, :3]).max() <= 2.0 ** -24, k                             # R: a double product rounded to float once


def test_failed_call_leaves_the_map_untouched():
    res, calls, log, err = run("member", QSP_STUB_FAIL="essential")
    assert res["status"] != 0 and calls == [] and log == []
    for k in range(8):
        assert res["kf"][k]["n"] == 0 and np.array_equal(res["kf"][k]["v"].reshape(4, 4), tcw(k).astype(np.float64))
    assert all(res["mp"][i]["n"] == 0 for i in range(5))
    assert res["failures"] == 1 and res["fallbacks"] == 0 and "the map is left untouched" in err


def test_default_dropin_still_reaches_g2o():
    res, calls, log, _ = run("dropin")
    assert calls == [] and [l.split()[0] for l in log] == ["g2o:OptimizeEssentialGraph"]
    assert all(res["kf"][k]["n"] == 0 for k in range(8)) and res["failures"] == 0


def test_opt_in_reaches_the_library_and_the_failure_row():
    res, calls, log, _ = run("dropin", QSP_SHIM_ESSENTIAL_HIP="1")
    assert len(calls) == 1 and log == [] and calls[0]["fix"] == 0 and calls[0]["n_edge"] == len(EDGES)
    assert res["kf"][0]["n"] == 1 and res["failures"] == 0
    res, calls, log, err = run("dropin", QSP_SHIM_ESSENTIAL_HIP="1", QSP_STUB_FAIL="essential")
    assert log == [] and all(res["kf"][k]["n"] == 0 for k in range(8)) and res["failures"] == 1 and res["fallbacks"] == 0
    res, calls, log, err = run("dropin", QSP_SHIM_ESSENTIAL_HIP="1", QSP_STUB_FAIL="essential", QSP_SHIM_ALLOW_G2O_FALLBACK="1")
    assert [l.split()[0] for l in log] == ["g2o:OptimizeEssentialGraph"] and res["failures"] == 1 and res["fallbacks"] == 1
    assert "falls back" in err
