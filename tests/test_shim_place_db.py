"""CPU: KeyFrameDatabaseHip (include/qsp_optimizer_shim.h), compiled against the stand-in map types of tests/shim_mock_place/ and a
stub of the qsp_place_db calls that records what it is given and answers with a fixed pattern.  A stand-alone program (sanitised),
never loaded into Python."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_place")
_EXE = {}


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_place_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc
                          + ["-c", os.path.join(MOCK, "place_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_place.c"),
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
                if k in ("create", "destroy", "put", "list", "erase", "clear", "query", "acc"):
                    calls.append(dict(call=k, args=[float(x) if "." in x or "e" in x else int(x) for x in v]))
                else:
                    calls[-1][k] = [float(x) for x in v] if k == "value" else [int(x) for x in v]
    res = {}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        res.setdefault(k, []).append([int(x) for x in v])
    return res, calls, r.stderr


# ---- the caller's procedural scene, restated -------------------------------------------------------------------------------------
def words(k):
    return sorted({k, k + 3, 2 * k + 7})


def ordered(k):
    return [10 + (k + d) % 6 for d in range(1, 14) if (k + d) % 6 != k]


def check_setup(calls):
    """add 3 0 2 4 1, erase 2, erase 5: every put hands over the BoW vector in map order"""
    assert calls[0]["call"] == "create" and calls[0]["args"][1:] == [0, 0]
    puts = calls[1:6]
    for c, k in zip(puts, (3, 0, 2, 4, 1)):
        assert c["call"] == "put" and c["args"] == [10 + k, 3, 1]
        assert c["word"] == words(k) and c["value"] == [(w + 1) / 64.0 for w in words(k)]
    assert [(c["call"], c["args"]) for c in calls[6:8]] == [("erase", [12]), ("erase", [15])]
    return calls[8:]


def test_loop_candidates_with_a_given_minimum_score():
    res, calls, _ = run("loop")
    assert res["status"] == [[0]] and res["failures"] == [[0]]
    rest = check_setup(calls)
    assert [c["call"] for c in rest] == ["query", "acc", "destroy"]
    q, a = rest[0], rest[1]
    assert q["args"] == [0, 3, 2, 0, 0.125, 0]                         # LOOP, 3 words, 2 excluded, no refs, the score, no taps
    assert q["word"] == words(5) and q["value"] == [(w + 1) / 64.0 for w in words(5)]
    assert sorted(q["excluded"]) == [10, 11] and q["ref"] == []       # the connected key frames
    # the stub's lScoreAndMatch: the listed ids in add() order less the excluded ones; neighbour lists for exactly those, cut at 10
    assert a["args"] == [0, 2] and a["id"] == [13, 14]
    assert a["off"] == [0, 10, 20] and a["nbr"] == ordered(3)[:10] + ordered(4)[:10] and len(ordered(3)) == 11
    assert res["candidates"] == [[14, 13]]                            # the stub's answer (reversed), mapped back to pointers in order
    assert res["best_calls"] == [[0, 0, 0, 1, 1, 0]]                  # GetBestCovisibilityKeyFrames only for the returned entries


def test_loop_candidates_with_detect_loops_minimum_in_the_same_call():
    res, calls, _ = run("loop_ref")
    assert res["status"] == [[0]] and res["failures"] == [[0]]
    rest = check_setup(calls)
    assert [c["call"] for c in rest] == ["put", "query", "acc", "query", "acc", "destroy"]
    p, q, a = rest[0], rest[1], rest[2]
    assert p["args"] == [15, 3, 0] and p["word"] == words(5)           # the covisible the database had not seen: known, NOT listed
    assert q["args"] == [0, 3, 3, 2, 1.0, 0] and q["word"] == words(0)
    assert sorted(q["excluded"]) == [11, 12, 15] and q["ref"] == [15, 11]      # refs: the non-bad covisibles in order (12 is bad)
    assert a["id"] == [13, 10, 14] and a["off"] == [0, 10, 13, 23] and a["nbr"] == ordered(3)[:10] + [12, 15, 11] + ordered(4)[:10]
    assert res["candidates"] == [[14, 10, 13]] and res["again"] == [[14, 10, 13]]
    assert rest[3]["ref"] == [15, 11]


def test_relocalisation_candidates():
    res, calls, _ = run("reloc")
    rest = check_setup(calls)
    assert [c["call"] for c in rest] == ["query", "acc", "destroy"]
    q, a = rest[0], rest[1]
    assert q["args"][:4] == [1, 3, 0, 0] and q["word"] == [1, 4, 9] and q["value"] == [0.5, 0.25, 0.25]     # map order, not insertion order
    assert a["args"] == [1, 4] and a["id"] == [13, 10, 14, 11] and a["off"] == [0, 10, 20, 30, 40]
    assert res["candidates"] == [[11, 14, 10, 13]] and res["best_calls"] == [[1, 1, 0, 1, 1, 0]]


def test_an_empty_database_and_the_life_cycle():
    res, calls, _ = run("empty")
    assert [c["call"] for c in calls] == ["create", "query", "destroy"] and res["candidates"] == [[]]       # no entries: no accumulate
    res, calls, _ = run("lifecycle")
    rest = check_setup(calls)
    assert [(c["call"], c["args"][:1]) for c in rest[:3]] == [("put", [15]), ("clear", []), ("put", [11])]
    assert [c["call"] for c in rest] == ["put", "clear", "put", "query", "acc", "destroy"]               # the repeated add made no call
    assert res["status"] == [[0], [0], [0], [0], [0]] and res["candidates"] == [[11]] and res["failures"] == [[0]]


def test_a_failed_call_leaves_an_empty_candidate_list_and_a_logged_error():
    for mode, what, name in (("loop", "query", "qsp_place_db_query"), ("reloc", "acc", "qsp_place_db_accumulate"),
                             ("loop_ref", "query", "qsp_place_db_query")):
        res, calls, err = run(mode, QSP_STUB_FAIL=what)
        assert res["candidates"] == [[]] and res["failures"][0][0] >= 1
        assert "%s failed" % name in err and "injected by the test stub" in err
    res, calls, err = run("loop", QSP_STUB_FAIL="put")
    assert res["status"] == [[3]] and "qsp_place_db_put failed" in err and res["candidates"] == [[]]
