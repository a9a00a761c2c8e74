"""CPU: OrbMatcherHip::SearchForTriangulationBatch (include/qsp_optimizer_shim.h), compiled against the stand-in map types of
tests/shim_mock_triangulation/ and a stub of qsp_search_for_triangulation_batch that records what it is given and answers with a
fixed pattern.  A stand-alone program (sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_triangulation")
_EXE = {}
f32 = np.float32
FLOATS = ("angle", "xy", "sigma2", "scale", "F12", "exy")


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_tri_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc
                          + ["-c", os.path.join(MOCK, "triangulation_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c",
                                                              os.path.join(MOCK, "stub_triangulation.c"), "-o", o("stub.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("stub.o")])
    _EXE["exe"] = o("caller")
    return _EXE["exe"]


def run(mode, **env_extra):
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
                    calls.append(dict(zip(("n_cand", "th", "only_stereo", "ori", "tap"), map(int, v)), frames=[]))
                elif k == "frame":
                    calls[-1]["frames"].append(dict(zip(("n", "n_nodes", "has_elig"), map(int, v))))
                else:
                    (calls[-1]["frames"][-1] if calls[-1]["frames"] else calls[-1])[k] = np.array(v, f32 if k in FLOATS else np.int64)
    res = dict(pairs=[])
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "pairs":
            res["pairs"].append([(int(a), int(b)) for a, b in zip(v[::2], v[1::2])])
        else:
            res[k] = [int(x) for x in v]
    return res, calls, r.stderr


# ---- the caller's procedural scene, restated in float32 ----------------------------------------------------------------------
N = {1: 10, 2: 6, 3: 0, 4: 8}
FILLED = (2, 4)                                                 # slot 2 holds a BAD map point, slot 4 a good one; every other is null


def check_kf(got, k):
    n = N[k]
    nodes = {}
    for j in range(n - 1, -1, -1):                              # the lists are in descending index order: passed on as they are
        nodes.setdefault(3 * (j % 4) + k, []).append(j)
    ids = sorted(nodes)
    assert (got["n"], got["n_nodes"], got["has_elig"]) == (n, len(ids), 1)
    assert list(got["desc"]) == [(j * 7 + b * 3 + k) % 256 for j in range(n) for b in range(32)]
    assert np.array_equal(got["angle"], np.array([f32(10) * f32(j) + f32(k) + f32(0.5) for j in range(n)], f32))
    assert list(got["elig"]) == [int(j not in FILLED) for j in range(n)]          # from null only: the bad point is NOT eligible
    assert list(got["node_id"]) == ids
    assert list(got["node_off"]) == list(np.concatenate([[0], np.cumsum([len(nodes[i]) for i in ids])]))
    assert list(got["feat"]) == [j for i in ids for j in nodes[i]]
    if n > 4:
        assert got["feat"][0] > got["feat"][1]
    xy = [v for j in range(n) for v in (f32(1.5) * f32(j) + f32(k), f32(2.25) * f32(j) - f32(k))]
    assert np.array_equal(got["xy"], np.array(xy, f32))
    assert list(got["stereo"]) == [int(j % 3 == 0) for j in range(n)]             # mvuRight[j] >= 0
    scale = [f32(1) + f32(0.25) * f32(l) + f32(0.01) * f32(k) for l in range(4)]
    sigma2 = [f32(2) + f32(l) + f32(0.5) * f32(k) for l in range(4)]
    assert np.array_equal(got["scale"], np.array([scale[(j + k) % 4] for j in range(n)], f32))      # through the octave
    assert np.array_equal(got["sigma2"], np.array([sigma2[(j + k) % 4] for j in range(n)], f32))
    if n > 4:
        assert len(set(got["scale"].tolist())) == 4 and len(set(got["sigma2"].tolist())) == 4


def epipole(k2):
    """:664-670 with key frame 1's centre; R2w * Cw as cv::Mat multiplies CV_32F: the row summed in double, rounded once"""
    Cw = [f32(0.37) * f32(r + 1) - f32(0.11) * f32(1) for r in range(3)]
    C2 = []
    for r in range(3):
        R = [(f32(0.9) if r == c else f32(0.1) * f32(r - c)) + f32(0.01) * f32(k2) for c in range(3)]
        t = f32(0.3) * f32(r) - f32(0.2) * f32(k2) + f32(1.7)
        C2.append(f32(f32(sum(float(R[c]) * float(Cw[c]) for c in range(3))) + t))
    fx, fy = f32(500) + f32(k2), f32(510) + f32(k2)
    cx, cy = f32(320) + f32(0.5) * f32(k2), f32(240) - f32(0.25) * f32(k2)
    invz = f32(1.0) / C2[2]
    return [fx * C2[0] * invz + cx, fy * C2[1] * invz + cy]


def expected_pairs():
    want = []
    for c, k2 in enumerate((2, 3, 4)):                          # the stub's pattern
        want.append([(i, (2 * i + c) % N[k2]) for i in range(N[1]) if N[k2] and i % 2 == c % 2 and i not in FILLED])
    return want


def test_one_call_with_everything_gathered():
    res, calls, _ = run("tri")
    assert res["status"] == [0] and len(calls) == 1             # one library call
    call = calls[0]
    assert (call["n_cand"], call["th"], call["only_stereo"], call["ori"], call["tap"]) == (3, 50, 0, 0, 0)
    assert len(call["frames"]) == 4
    for got, k in zip(call["frames"], (1, 2, 3, 4)):
        check_kf(got, k)
    assert np.array_equal(call["F12"], np.array([10 * c + 3 * r + q + 0.5 for c in range(3) for r in range(3) for q in range(3)], f32))
    want_e = np.array([v for k2 in (2, 3, 4) for v in epipole(k2)], f32)
    assert np.array_equal(call["exy"], want_e) and np.isfinite(want_e).all() and len(set(want_e.tolist())) == 6
    want = expected_pairs()
    assert res["pairs"] == want and res["counts"] == [100, 101, 102]
    assert len(want[0]) >= 2 and want[1] == [] and len(want[2]) >= 2
    for p in want:
        assert [a for a, _ in p] == sorted(a for a, _ in p)     # ascending idx1


def test_the_flags_are_passed_on():
    res, calls, _ = run("stereo")
    assert res["status"] == [0] and len(calls) == 1
    assert (calls[0]["only_stereo"], calls[0]["ori"], calls[0]["th"]) == (1, 1, 50) and res["pairs"] == expected_pairs()


def test_a_failed_call_leaves_the_outputs_untouched():
    res, calls, err = run("tri", QSP_STUB_FAIL="tri")
    assert res["status"] == [3] and calls == [] and res["counts"] == [-4] and res["pairs"] == [[(900, 901)]]
    assert "qsp_search_for_triangulation_batch failed" in err


def test_an_empty_neighbour_list_makes_no_call():
    res, calls, _ = run("empty")
    assert res["status"] == [0] and calls == [] and res["counts"] == [] and res["pairs"] == []
