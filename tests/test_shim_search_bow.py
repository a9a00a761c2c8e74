"""CPU: both OrbMatcherHip::SearchByBoWBatch overloads (include/qsp_optimizer_shim.h), compiled against the stand-in map types of
tests/shim_mock_bow/ and a stub of qsp_search_by_bow_batch that records what it is given and answers with a fixed pattern.  A
stand-alone program (sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_bow")
_EXE = {}
f32 = np.float32


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_bow_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc
                          + ["-c", os.path.join(MOCK, "bow_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_bow.c"),
                                                              "-o", o("stub.o")])
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
                    calls.append(dict(zip(("n_cand", "sis", "th", "th_inclusive", "ori", "tap"), map(int, v)), frames=[]))
                elif k == "nn":
                    calls[-1]["nn"] = f32(v[0])
                elif k == "frame":
                    calls[-1]["frames"].append(dict(zip(("n", "n_nodes", "has_elig"), map(int, v))))
                else:
                    calls[-1]["frames"][-1][k] = np.array(v, f32 if k == "angle" else np.int64)
    res = dict(matches=[])
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "matches":
            res["matches"].append([int(x) for x in v])
        else:
            res[k] = [int(x) for x in v]
    return res, calls, r.stderr


# ---- the caller's procedural scene, restated ---------------------------------------------------------------------------------
N = {1: 10, 2: 6, 3: 0, 4: 8}
NF = 7


def check_kf(got, k):
    n = N[k]
    nodes = {}
    for j in range(n - 1, -1, -1):                              # the lists are in descending index order: passed on as they are
        nodes.setdefault(3 * (j % 4) + k, []).append(j)
    ids = sorted(nodes)
    assert (got["n"], got["n_nodes"], got["has_elig"]) == (n, len(ids), 1)
    assert list(got["desc"]) == [(j * 7 + b * 3 + k) % 256 for j in range(n) for b in range(32)]
    assert np.array_equal(got["angle"], np.array([f32(10) * f32(j) + f32(k) + f32(0.5) for j in range(n)], f32))
    assert list(got["elig"]) == [int(j not in (1, 2)) for j in range(n)]          # a null slot and a bad map point are not eligible
    assert list(got["node_id"]) == ids
    assert list(got["node_off"]) == list(np.concatenate([[0], np.cumsum([len(nodes[i]) for i in ids])]))
    assert list(got["feat"]) == [j for i in ids for j in nodes[i]]
    if n > 4:
        assert list(got["feat"][:2]) == sorted(got["feat"][:2], reverse=True) and got["feat"][0] > got["feat"][1]


def check_frame(got):
    assert (got["n"], got["n_nodes"], got["has_elig"]) == (NF, 3, 0) and len(got["elig"]) == 0    # NULL eligibility in frame mode
    assert list(got["desc"]) == [(j * 5 + b) % 256 for j in range(NF) for b in range(32)]
    assert np.array_equal(got["angle"], np.array([f32(3) * f32(j) + f32(0.25) for j in range(NF)], f32))
    assert list(got["node_id"]) == [0, 2, 4] and list(got["node_off"]) == [0, 3, 5, 7] and list(got["feat"]) == [0, 3, 6, 1, 4, 2, 5]


def mp_id(k, j):
    return -1 if j == 1 else 100 * k + j                        # slot 1 of every key frame is null


def test_loop_closing_overload():
    res, calls, _ = run("kf")
    assert res["status"] == [0] and len(calls) == 1             # one library call
    call = calls[0]
    assert (call["n_cand"], call["sis"], call["th"], call["th_inclusive"], call["ori"], call["tap"]) == (3, 1, 50, 0, 1, 0)
    assert call["nn"] == f32(0.75) and len(call["frames"]) == 4
    for got, k in zip(call["frames"], (1, 2, 3, 4)):
        check_kf(got, k)
    want = []
    for c, k2 in enumerate((2, 3, 4)):                          # the stub's pattern, written back as key frame 2's map points
        row = [-1] * N[1]
        for i in range(N[1]):
            if N[k2] and i % 2 == c % 2 and i not in (1, 2):
                row[i] = mp_id(k2, (2 * i + c) % N[k2])
        want.append(row)
    assert res["matches"] == want and res["counts"] == [100, 101, 102]
    assert any(x >= 0 for x in want[0]) and all(x == -1 for x in want[1]) and any(x >= 0 for x in want[2])


def test_relocalisation_overload_inverts_the_result():
    res, calls, _ = run("frame")
    assert res["status"] == [0] and len(calls) == 1
    call = calls[0]
    assert (call["n_cand"], call["sis"], call["th"], call["th_inclusive"], call["ori"], call["tap"]) == (3, 0, 50, 1, 0, 0)
    assert call["nn"] == f32(0.9) and len(call["frames"]) == 4
    check_frame(call["frames"][0])                              # the frame is the shared one; then one key frame per candidate
    for got, k in zip(call["frames"][1:], (2, 3, 4)):
        check_kf(got, k)
    want = []
    for c, k in enumerate((2, 3, 4)):                           # source slot i -> frame key point idxF, inverted: [idxF] = point of slot i
        row = [-1] * NF
        for i in range(N[k]):
            if i % 2 == c % 2 and i not in (1, 2):
                row[(2 * i + c) % NF] = mp_id(k, i)
        want.append(row)
    assert res["matches"] == want and res["counts"] == [100, 101, 102]
    assert sum(x >= 0 for x in want[0]) >= 2 and sum(x >= 0 for x in want[2]) >= 2


def test_a_failed_call_leaves_the_outputs_untouched():
    for mode in ("kf", "frame"):
        res, calls, err = run(mode, QSP_STUB_FAIL="bow")
        assert res["status"] == [3] and calls == [] and res["counts"] == [-4] and res["matches"] == [[900]]
        assert "qsp_search_by_bow_batch failed" in err


def test_an_empty_candidate_list_makes_no_call():
    for mode in ("kf_empty", "frame_empty"):
        res, calls, _ = run(mode)
        assert res["status"] == [0] and calls == [] and res["counts"] == [] and res["matches"] == []
