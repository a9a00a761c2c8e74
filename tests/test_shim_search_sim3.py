"""CPU: OrbMatcherHip::SearchBySim3Batch (include/qsp_optimizer_shim.h), compiled against the stand-in map types of
tests/shim_mock_search/ and a stub of qsp_search_by_sim3_batch that records what it is given and answers with a fixed pattern.  A
stand-alone program (sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_search")
_EXE = {}
f32 = np.float32


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_search_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc
                          + ["-c", os.path.join(MOCK, "search_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_search.c"),
                                                              "-o", o("stub.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("stub.o")])
    _EXE["exe"] = o("caller")
    return _EXE["exe"]


INT_KEYS = ("off2", "pre1", "pre2", "octave", "desc", "has", "mpd")


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
                    calls.append(dict(zip(("n_cand", "n1", "tap"), map(int, v)), frames=[]))
                    at = calls[-1]
                elif k == "frame":
                    calls[-1]["frames"].append(dict(zip(("n", "cols", "rows", "n_levels"), map(int, v))))
                    at = calls[-1]["frames"][-1]
                else:
                    at[k] = np.array(v, np.int64 if k in INT_KEYS else np.float32)
    res = dict(matches=[])
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "matches":
            res["matches"].append([int(x) for x in v])
        else:
            res[k] = [int(x) for x in v]
    return res, calls, r.stderr


# ---- the caller's procedural scene, restated ---------------------------------------------------------------------------------
N1, N2 = 12, (8, 0, 10)


MIX = {2: (5, 7, 5, 1.5, 0.4055), 3: (64, 64, 16, 1.1, 0.0953), 4: (1, 1, 1, 1.3, 0.2624)}   # cols, rows, levels, scale, log_scale


def frame(k, n, mixed=False):
    cols, rows, levels, scale, log_scale = MIX[k] if mixed else (64, 48, 4, 1.2, 0.1823)
    a = 0.1 * k
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).astype(f32)
    t = np.array([f32(0.1) * f32(r + 1) * f32(k) for r in range(3)], f32)
    sf, s = [], f32(1)
    for _ in range(levels):
        sf.append(s)
        s = f32(s * f32(scale))
    par = [-k, 640 + k, -2 * k, 480 + k, f32(cols) / f32(640 + 2 * k), f32(rows) / f32(480 + 3 * k), f32(log_scale)]
    return dict(R=R.reshape(-1), t=t, sf=np.array(sf, f32), par=np.array(par, f32), shape=(cols, rows, levels),
                kp=np.array([[f32(7) * f32(j) + f32(k), f32(5) * f32(j) + f32(2) * f32(k)] for j in range(n)], f32).reshape(-1),
                octave=np.array([j % levels for j in range(n)]),
                desc=np.array([[(j * 7 + b * 3 + k) % 256 for b in range(32)] for j in range(n)]).reshape(-1))


def point(pid, i, dy):
    maxd = f32(f32(3) + f32(0.25) * f32(i)) + f32(0.01) * f32(pid)
    return dict(X=[f32(0.1) * f32(i) - f32(0.5), f32(0.05) * f32(i) + f32(dy), f32(2) + f32(0.3) * f32(i)],
                dmin=f32(0.8) * f32(maxd / f32(2)), dmaxi=f32(1.2) * maxd, dmax=f32(f32(1.2) * maxd) / f32(1.2),
                mpd=[(pid * 5 + b) % 256 for b in range(32)], id=pid)


def slots(n, base, dy, null, bad):
    """per slot: the point dict or None, and has_point"""
    return [(None if j == null else point(base + j, j, dy)) for j in range(n)], [int(j not in (null, bad)) for j in range(n)]


def check_frame(got, k, n, pts, has, mixed=False):
    e = frame(k, n, mixed)
    assert (got["n"], got["cols"], got["rows"], got["n_levels"]) == (n,) + e["shape"] and len(got["sf"]) == e["shape"][2]
    for key, want in (("par", e["par"]), ("sf", e["sf"]), ("Rcw", e["R"]), ("tcw", e["t"]), ("kp", e["kp"])):
        assert np.array_equal(got[key], want), (k, key, got[key], want)
    assert list(got["octave"]) == list(e["octave"]) and list(got["desc"]) == list(e["desc"]) and list(got["has"]) == has
    for j, (p, h) in enumerate(zip(pts, has)):
        if not h:                                              # a null or bad point: its other fields are zeros
            assert not got["Xw"][3 * j:3 * j + 3].any() and got["dmax"][j] == 0 and not got["mpd"][32 * j:32 * j + 32].any()
            continue
        assert np.array_equal(got["Xw"][3 * j:3 * j + 3], np.array(p["X"], f32)), (k, j)
        assert got["dmin"][j] == p["dmin"] and got["dmaxi"][j] == p["dmaxi"] and got["dmax"][j] == p["dmax"], (k, j)   # getter / 1.2f
        assert list(got["mpd"][32 * j:32 * j + 32]) == p["mpd"]


def test_gathered_arrays():
    res, calls, _ = run()
    assert res["status"] == [0] and len(calls) == 1             # one call
    call = calls[0]
    assert (call["n_cand"], call["n1"], call["tap"]) == (3, N1, 0)
    assert len(call["frames"]) == 4                             # key frame 1 once, then one frame per candidate
    check_frame(call["frames"][0], 1, N1, *slots(N1, 0, 0.0, 3, 5))
    for c in range(3):
        check_frame(call["frames"][1 + c], 2 + c, N2[c], *slots(N2[c], 100 * (c + 1), 0.1 * c, 1, 2))
    assert list(call["off2"]) == [0, 8, 8, 18]
    k1 = [f32(501), f32(511), f32(320.5), f32(240.25)]          # key frame 1's intrinsics for every candidate
    assert np.array_equal(call["K"], np.array(k1 * 3, f32))
    assert np.array_equal(call["s12"], np.array([1.1, 0.9, 1.25], f32)) and np.array_equal(call["th"], np.full(3, 7.5, f32))
    assert np.array_equal(call["R12"], np.array([10 * c + 3 * r + q for c in range(3) for r in range(3) for q in range(3)], f32))   # row-major
    assert np.array_equal(call["t12"], np.array([0.5 * c + r for c in range(3) for r in range(3)], f32))
    pre1 = np.zeros((3, N1), int)
    pre1[0, 4] = pre1[0, 7] = pre1[1, 2] = pre1[2, 0] = 1
    pre2 = np.zeros(18, int)
    pre2[6] = 1                                                 # candidate 0: slot 6; the foreign point of slot 7 has no index: pre1 only
    pre2[8 + 9] = 1
    assert list(call["pre1"]) == list(pre1.reshape(-1)) and list(call["pre2"]) == list(pre2)


def test_every_frame_is_marshalled_with_its_own_pyramid_and_grid():
    """mode "mixed": 5 x 7 cells with 5 levels at 1.5, 64 x 64 with 16 at 1.1, 1 x 1 with 1 level, next to key frame 1's 64 x 48
    with 4 at 1.2 -- each qsp_orb_frame holds its own frame's values, not key frame 1's and not a neighbour's"""
    res, calls, _ = run("mixed")
    assert res["status"] == [0] and len(calls) == 1 and len(calls[0]["frames"]) == 4
    fr = calls[0]["frames"]
    check_frame(fr[0], 1, N1, *slots(N1, 0, 0.0, 3, 5))
    for c in range(3):
        check_frame(fr[1 + c], 2 + c, N2[c], *slots(N2[c], 100 * (c + 1), 0.1 * c, 1, 2), mixed=True)
    assert [(f["cols"], f["rows"], f["n_levels"]) for f in fr] == [(64, 48, 4), (5, 7, 5), (64, 64, 16), (1, 1, 1)]
    assert len({float(f["par"][6]) for f in fr}) == 4 and len({float(f["par"][4]) for f in fr}) == 4       # log_scale, width_inv
    assert np.array_equal(fr[2]["sf"][:3], np.array([1, f32(1.1), f32(1.1) * f32(1.1)], f32))
    m, found = expected_matches()                              # the write-back does not depend on any of it
    assert res["matches"] == m and res["found"] == found


def expected_matches():
    ids = lambda c, j: -1 if j == 1 else 100 * (c + 1) + j       # slot 1 of every key frame 2 is null
    m = [[-1] * N1 for _ in range(3)]
    m[0][4], m[0][7], m[1][2], m[2][0] = 106, 900, 900, 309
    found = [0, 0, 0]
    for c in range(3):
        for i1 in range(N1):
            if N2[c] and i1 % 3 == c % 3 and m[c][i1] == -1:
                m[c][i1] = ids(c, (i1 + c) % N2[c])
                found[c] += 1
    return m, found


def test_write_back_of_the_agreed_slots():
    res, _, _ = run()
    m, found = expected_matches()
    assert res["matches"] == m and res["found"] == found and found == [4, 0, 4]


def test_a_failed_call_leaves_the_outputs_untouched():
    res, calls, err = run(QSP_STUB_FAIL="search")
    assert res["status"] == [3] and calls == [] and res["found"] == [-4, -4, -4]
    before = [[-1] * N1 for _ in range(3)]
    before[0][4], before[0][7], before[1][2], before[2][0] = 106, 900, 900, 309
    assert res["matches"] == before
    assert "qsp_search_by_sim3_batch failed" in err
    res, calls, err = run("short")                              # an argument vector of the wrong length: refused before any call
    assert res["status"] == [1] and calls == [] and res["found"] == [-4, -4, -4] and res["matches"] == before
