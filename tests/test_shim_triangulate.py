"""CPU: OrbMatcherHip::CreateNewMapPointsBatch and TriangulateBatch (include/qsp_optimizer_shim.h), compiled against the stand-in
map types of tests/shim_mock_create_points/ and a stub of qsp_create_new_map_points_batch and qsp_triangulate_batch that records
what it is given and answers with a fixed pattern.  A stand-alone program (sanitised), never loaded into Python.  What the search
half gathers (descriptors, feature vectors, eligibility) is tests/test_shim_search_triangulation.py's; here F12, the epipoles and
the frame sizes show that the same gather feeds the chained call."""
import os
import subprocess
import tempfile

import numpy as np

from tests import test_shim_search_triangulation as search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_create_points")
_EXE = {}
f32 = np.float32
INTS = ("search_n", "match")


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_create_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc
                          + ["-c", os.path.join(MOCK, "create_points_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c",
                                                              os.path.join(MOCK, "stub_create_points.c"), "-o", o("stub.o")])
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
                    calls.append(dict(zip(("n_cand", "th", "only_stereo", "ori", "tap"), map(int, v[1:])), which=v[0], frames=[]))
                elif k == "geom":
                    calls[-1].update(geom_n=int(v[0]), ratio_factor=f32(v[1]))
                elif k == "gframe":
                    calls[-1]["frames"].append(dict(n=int(v[0])))
                else:
                    (calls[-1]["frames"][-1] if calls[-1]["frames"] else calls[-1])[k] = np.array(v, np.int64 if k in INTS else f32)
    res = dict(new=[])
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "new":
            res["new"].append((int(v[0]), int(v[1]), int(v[2]), (int(v[3]), int(v[4])), [f32(x) for x in v[5:]]))
        else:
            res[k] = [int(x) for x in v]
    return res, calls, r.stderr


# ---- the caller's procedural scene, restated in float32 ----------------------------------------------------------------------
N = {1: 10, 2: 6, 3: 0, 4: 8}
FILLED = (4,)


def check_geometry(got, k):
    n, K = N[k], f32(k)
    assert got["n"] == n
    R = [(f32(0.9) if r == c else f32(0.1) * f32(r - c)) + f32(0.01) * K for r in range(3) for c in range(3)]
    assert np.array_equal(got["Rcw"], np.array(R, f32))                                             # GetRotation, row-major
    assert np.array_equal(got["tcw"], np.array([f32(0.3) * f32(r) - f32(0.2) * K + f32(1.7) for r in range(3)], f32))
    assert np.array_equal(got["Ow"], np.array([f32(0.37) * f32(r + 1) - f32(0.11) * K for r in range(3)], f32))   # GetCameraCenter, not -R't
    cam = [f32(500) + K, f32(510) + K, f32(320) + f32(0.5) * K, f32(240) - f32(0.25) * K, f32(0.002) + f32(0.0001) * K,
           f32(0.003) - f32(0.0001) * K, f32(0.08) + f32(0.01) * K, f32(40) + K]
    assert np.array_equal(got["K"], np.array(cam, f32))                                             # invfx, invfy READ; mb beside mbf
    assert cam[4] != f32(1) / cam[0] and cam[7] != cam[6] * cam[0]
    J = [f32(j) for j in range(n)]
    un = [v for j in J for v in (f32(1.5) * j + K, f32(2.25) * j - K)]
    raw = [v for j in J for v in (f32(1.5) * j + K + f32(0.75), f32(2.25) * j - K - f32(0.375))]
    assert np.array_equal(got["xy_un"], np.array(un, f32)) and np.array_equal(got["xy"], np.array(raw, f32))   # mvKeysUn against mvKeys
    assert np.array_equal(got["u_right"], np.array([f32(5) + j if int(j) % 3 == 0 else f32(-1) for j in J], f32))
    assert np.array_equal(got["depth"], np.array([f32(3) + f32(0.5) * j + K if int(j) % 3 == 0 else f32(-1) for j in J], f32))
    scale = [f32(1) + f32(0.25) * f32(l) + f32(0.01) * K for l in range(4)]
    sigma2 = [f32(2) + f32(l) + f32(0.5) * K for l in range(4)]
    assert np.array_equal(got["scale"], np.array([scale[(j + k) % 4] for j in range(n)], f32))      # through mvKeysUn's octave,
    assert np.array_equal(got["sigma2"], np.array([sigma2[(j + k) % 4] for j in range(n)], f32))    # not mvKeys' (which is one further)
    if n > 4:
        assert len(set(got["scale"].tolist())) == 4 and len(set(got["sigma2"].tolist())) == 4
        assert not np.array_equal(got["xy"], got["xy_un"]) and (got["depth"][got["u_right"] >= 0] > 0).all()


def x3d(k, i, idx2):
    return [f32(k + 0.5), f32(i + 0.25), f32(idx2 + 0.125)]


def expected_new():
    """the stub's pattern: the search half's matches (an eligible slot i of the same parity as the neighbour), `first` unless
    i % 3 == 2; neighbour first, then ascending idx1"""
    want = []
    for c, k2 in enumerate((2, 3, 4)):
        for i in range(N[1]):
            if N[k2] and i % 2 == c % 2 and i not in FILLED and i % 3 != 2:
                want.append((c, i, (2 * i + c) % N[k2], (3, 1), x3d(c, i, (2 * i + c) % N[k2])))
    return want


def test_one_chained_call_with_everything_gathered():
    res, calls, _ = run("create")
    assert res["status"] == [0] and len(calls) == 1 and calls[0]["which"] == "create"                # one library call
    call = calls[0]
    assert (call["n_cand"], call["th"], call["only_stereo"], call["ori"], call["tap"]) == (3, 50, 0, 0, 0)
    assert call["geom_n"] == 3 and call["ratio_factor"] == f32(1.5) * (f32(1.2) + f32(0.05) * f32(1))   # 1.5f * key frame 1's mfScaleFactor
    assert list(call["search_n"]) == [N[k] for k in (1, 2, 3, 4)] and len(call["frames"]) == 4
    for got, k in zip(call["frames"], (1, 2, 3, 4)):
        check_geometry(got, k)
    assert np.array_equal(call["F12"], np.array([10 * c + 3 * r + q + 0.5 for c in range(3) for r in range(3) for q in range(3)], f32))
    assert np.array_equal(call["exy"], np.array([v for k2 in (2, 3, 4) for v in search.epipole(k2)], f32))
    want = expected_new()
    assert res["new"] == want and res["counts"] == [100, 101, 102]
    assert len([w for w in want if w[0] == 0]) >= 2 and not [w for w in want if w[0] == 1] and len([w for w in want if w[0] == 2]) >= 2
    assert [(w[0], w[1]) for w in want] == sorted((w[0], w[1]) for w in want)                        # neighbour first, then ascending idx1
    assert 2 not in [w[1] for w in want] and 8 not in [w[1] for w in want]                            # matched, accepted, but not first


def test_the_flags_are_passed_on():
    res, calls, _ = run("flags")
    assert res["status"] == [0] and len(calls) == 1
    assert (calls[0]["only_stereo"], calls[0]["ori"], calls[0]["th"]) == (1, 1, 50) and res["new"] == expected_new()


def test_the_plain_overload_builds_the_grid_from_the_lists():
    res, calls, _ = run("tri")
    assert res["status"] == [0] and len(calls) == 1 and calls[0]["which"] == "tri" and calls[0]["tap"] == 0
    grid = np.full((3, N[1]), -1)
    grid[0, [1, 3, 8]] = [5, 0, 2]
    grid[2, [0, 2, 9]] = [7, 1, 3]
    assert np.array_equal(calls[0]["match"], grid.reshape(-1))
    for got, k in zip(calls[0]["frames"], (1, 2, 3, 4)):
        check_geometry(got, k)
    assert calls[0]["ratio_factor"] == f32(1.5) * (f32(1.2) + f32(0.05))
    assert res["new"] == [(0, 1, 5, (3, 1), x3d(0, 1, 5)), (0, 3, 0, (3, 1), x3d(0, 3, 0)), (2, 0, 7, (3, 1), x3d(2, 0, 7)),
                          (2, 9, 3, (3, 1), x3d(2, 9, 3))]
    assert res["counts"] == [-4]                                                                       # the overload has no vnMatches


def test_a_failed_call_leaves_the_outputs_untouched():
    for mode, fail, name in (("create", "create", "qsp_create_new_map_points_batch"), ("tri", "tri", "qsp_triangulate_batch")):
        res, calls, err = run(mode, QSP_STUB_FAIL=fail)
        assert res["status"] == [3] and calls == [] and res["counts"] == [-4]
        assert [(n[0], n[1], n[2]) for n in res["new"]] == [(77, 78, 79)]                              # the sentinel point is still there
        assert "%s failed" % name in err


def test_an_empty_neighbour_list_makes_no_call():
    res, calls, _ = run("empty")
    assert res["status"] == [0] and calls == [] and res["counts"] == [] and res["new"] == []
