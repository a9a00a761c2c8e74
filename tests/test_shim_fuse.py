"""CPU: both OrbMatcherHip::FuseBatch overloads (include/qsp_optimizer_shim.h), compiled against the stand-in map types of
tests/shim_mock_fuse/ and a stub of qsp_fuse_batch that records what it is given and answers from a script.  A stand-alone program
(sanitised), never loaded into Python.  The gathered arrays are restated here in float32; the replayed action phase is compared
with the map model of tests/fuse_oracle.py on scripted scenes."""
import os
import subprocess
import tempfile

import numpy as np

from tests import fuse_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_fuse")
_EXE = {}
f32, f64 = np.float32, np.float64
INTS = ("check", "u_right_off", "list_off", "list_idx", "pool_desc", "octave", "desc")


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_fuse_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc + ["-c", os.path.join(MOCK, "fuse_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_fuse.c"), "-o", o("stub.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("stub.o")])
    _EXE["exe"] = o("caller")
    return _EXE["exe"]


def run(scene, answers, **env_extra):
    """scene: dict(mode, th, callback, kfs [slots], points [None | bad], obs [(point, kf, slot)], targets [kf]); answers: {(k, a): (best, dist)}"""
    with tempfile.TemporaryDirectory() as tmp:
        lines = ["mode %s" % scene["mode"], "th %r" % scene["th"], "callback %d" % scene.get("callback", 0)]
        lines += ["kf %d" % n for n in scene["kfs"]]
        lines += ["pt null" if b is None else "pt %d" % b for b in scene["points"]]
        lines += ["obs %d %d %d" % o for o in scene["obs"]]
        lines.append("targets " + " ".join(str(k) for k in scene["targets"]))
        open(os.path.join(tmp, "scene.txt"), "w").write("\n".join(lines) + "\n")
        open(os.path.join(tmp, "answers.txt"), "w").write("".join("%d %d %d %d\n" % (k, a, b, d) for (k, a), (b, d) in answers.items()))
        env = {k: v for k, v in os.environ.items() if not k.startswith("QSP_")}
        env.update(QSP_STUB_DUMP=os.path.join(tmp, "dump.txt"), QSP_STUB_ANSWERS=os.path.join(tmp, "answers.txt"), **env_extra)
        r = subprocess.run([build(), os.path.join(tmp, "scene.txt")], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        calls = []
        if os.path.exists(env["QSP_STUB_DUMP"]):
            for line in open(env["QSP_STUB_DUMP"]).read().splitlines():
                k, *v = line.split()
                if k == "call":
                    calls.append(dict(zip(("n_target", "n_point", "tap"), map(int, v)), frames=[]))
                elif k == "frame":
                    calls[-1]["frames"].append(dict(zip(("n", "cols", "rows", "n_levels", "has_point"), map(int, v))))
                else:
                    (calls[-1]["frames"][-1] if calls[-1]["frames"] else calls[-1])[k] = np.array(v, np.int64 if k in INTS else f32)
    res = dict(replace=[], slots=[], points=[])
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k in ("replace", "slots"):
            res[k].append([None if int(x) < 0 else int(x) for x in v])
        elif k == "point":
            res["points"].append(None if v == ["null"] else (bool(int(v[0])), {int(o.split(":")[0]): int(o.split(":")[1]) for o in v[1:]}))
        else:
            res[k] = [int(x) for x in v]
    return res, calls, r.stderr


def model_of(scene):
    m = fo.MapModel({k: n for k, n in enumerate(scene["kfs"])})
    for i, b in enumerate(scene["points"]):
        if b is not None:
            m.point(i, bool(b))
    for p, k, slot in scene["obs"]:
        m.add(p, k, slot)
    return m, [None if b is None else i for i, b in enumerate(scene["points"])]


def lists_of(scene):
    m, pts = model_of(scene)
    if scene["mode"] == "pose":
        return fo.fuse_pose_model(m, scene["targets"], pts, [[(-1, -1)] * len(pts)] * len(scene["targets"]))[2]
    return fo.fuse_sim3_model(m, scene["targets"], pts, [[(-1, -1)] * len(pts)] * len(scene["targets"]))[2]


def scripted(scene, by_point):
    """by_point {(target position k, point): best_idx} -> the stub's script {(k, list position): (best, dist)} and the model's answers"""
    lists = lists_of(scene)
    answers = {(k, lists[k].index(p)): (b, 17) for (k, p), b in by_point.items()}
    per_target = [[answers.get((k, a), (-1, -1)) for a in range(len(lists[k]))] for k in range(len(lists))]
    return answers, per_target


def map_equals(res, m, pts):
    st = m.state()
    assert res["slots"] == [st["slots"][k] for k in sorted(st["slots"])]
    want = [None if p is None else (st["bad"][p], st["obs"][p]) for p in pts]
    assert res["points"] == want


# ---- what the caller's procedural key frames and points hold, restated in float32 -------------------------------------------------
def kf_expect(k, n):
    sf = [f32(1) + f32(0.25) * f32(l) + f32(0.01) * f32(k) for l in range(4)]
    inv = [f32(1) / (f32(2) + f32(l) + f32(0.5) * f32(k)) for l in range(4)]
    T = np.zeros((3, 4), f32)
    for r in range(3):
        for c in range(3):
            T[r, c] = (f32(0.9) if r == c else f32(0.1) * f32(r - c)) + f32(0.01) * f32(k)
        T[r, 3] = f32(0.3) * f32(r) - f32(0.2) * f32(k) + f32(1.7)
    return dict(K=[f32(500) + f32(k), f32(510) + f32(k), f32(320) + f32(0.5) * f32(k), f32(240) - f32(0.25) * f32(k), f32(40) + f32(k)], sf=sf, inv=inv,
                geom=[f32(-k), f32(640 + k), f32(0), f32(480), f32(64) / f32(640 + 2 * k), f32(48) / f32(480), f32(0.2) + f32(0.01) * f32(k)],
                kp=[v for j in range(n) for v in (f32(1.5) * f32(j) + f32(k), f32(2.25) * f32(j) - f32(k))], octave=[(j + k) % 4 for j in range(n)],
                u_right=[f32(5) + f32(j) if j % 3 == 0 else f32(-1) for j in range(n)], desc=[(j * 7 + b * 3 + k) % 256 for j in range(n) for b in range(32)],
                T=T, Ow=[f32(0.37) * f32(r + 1) - f32(0.11) * f32(k) for r in range(3)])


def check_gathered(scene, call, lists):
    tg, pts = scene["targets"], scene["points"]
    nt, npt = len(tg), len(pts)
    assert (call["n_target"], call["n_point"], call["tap"]) == (nt, npt, 0)
    e = [kf_expect(k, scene["kfs"][k]) for k in tg]
    assert np.array_equal(call["K"], np.array([v for x in e for v in x["K"]], f32))
    assert np.array_equal(call["th"], np.full(nt, scene["th"], f32))
    assert np.array_equal(call["inv_level_sigma2"], np.array([v for x in e for v in x["inv"] + [f32(0)] * 12], f32))
    assert list(call["check"]) == [int(scene["mode"] == "pose")] * nt
    assert list(call["u_right_off"]) == list(np.concatenate([[0], np.cumsum([scene["kfs"][k] for k in tg])]))
    assert np.array_equal(call["u_right"], np.array([v for x in e for v in x["u_right"]], f32))
    assert list(call["list_off"]) == list(np.concatenate([[0], np.cumsum([len(l) for l in lists])]))
    assert list(call["list_idx"]) == [i for l in lists for i in l]
    ok = [b is not None and not b for b in pts]
    z = lambda vals, w: np.array([v if ok[i] else f32(0) for i in range(npt) for v in vals(i)], f32).reshape(-1)
    assert np.array_equal(call["Xw"], z(lambda i: (f32(0.1) * f32(i) + f32(1), f32(0.2) * f32(i) - f32(1), f32(0.05) * f32(i) + f32(3)), 3))
    assert np.array_equal(call["normal"], z(lambda i: (f32(0.01) * f32(i), f32(0.02) * f32(i), f32(1) - f32(0.001) * f32(i)), 3))
    assert np.array_equal(call["dist_min_inv"], z(lambda i: (f32(0.8) * (f32(1) + f32(0.1) * f32(i)),), 1))
    dmaxi = z(lambda i: (f32(1.2) * (f32(10) + f32(i)),), 1)
    assert np.array_equal(call["dist_max_inv"], dmaxi) and np.array_equal(call["dist_max"], (dmaxi / f32(1.2)).astype(f32))
    assert list(call["pool_desc"]) == [(i * 5 + b) % 256 if ok[i] else 0 for i in range(npt) for b in range(32)]
    for x, k, fr in zip(e, tg, call["frames"]):
        assert (fr["n"], fr["cols"], fr["rows"], fr["n_levels"]) == (scene["kfs"][k], 64, 48, 4)
        assert np.array_equal(fr["geom"], np.array(x["geom"], f32)) and np.array_equal(fr["sf"], np.array(x["sf"], f32))
        assert np.array_equal(fr["kp"], np.array(x["kp"], f32)) and list(fr["octave"]) == x["octave"] and list(fr["desc"]) == x["desc"]
        if scene["mode"] == "pose":
            R, t, Ow = x["T"][:, :3], x["T"][:, 3], np.array(x["Ow"], f32)          # GetRotation, GetTranslation, GetCameraCenter
        else:
            # :986-990.  scw = sqrt(row 0 . row 0) summed in double; sRcw / scw as a float32 product with 1.0 / scw rounded to float32;
            # Ow = -Rcw.t() * tcw with each row summed in double and rounded once
            s = f32(1.5) + f32(0.25) * f32(k)
            S = (s * x["T"]).astype(f32)
            scw = f32(np.sqrt(sum(f64(S[0, c]) * f64(S[0, c]) for c in range(3))))
            inv = f32(1.0 / f64(scw))
            R, t = (S[:, :3] * inv).astype(f32), (S[:, 3] * inv).astype(f32)
            Ow = np.array([f32(-sum(f64(R[q, r]) * f64(t[q]) for q in range(3))) for r in range(3)], f32)
            assert abs(float(scw) / float(s) - np.linalg.norm(x["T"][0, :3].astype(f64))) < 1e-6
        assert np.array_equal(fr["Rcw"], R.reshape(9)) and np.array_equal(fr["tcw"], t)
        i = tg.index(k)
        assert np.array_equal(call["Ow"][3 * i:3 * i + 3], Ow)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
# point 2 is null, 3 and 10 are bad; 8 .. 11 start as occupants of the targets' slots
POSE = dict(mode="pose", th=3.0, kfs=[8, 6, 8, 5], points=[0, 0, None, 1, 0, 0, 0, 0, 0, 0, 1, 0], targets=[1, 2, 3],
            obs=[(0, 0, 0), (1, 0, 1), (1, 1, 2), (4, 0, 2), (5, 0, 3), (5, 3, 1), (6, 0, 4), (8, 1, 3), (8, 2, 1), (8, 3, 0), (9, 1, 4), (9, 2, 6), (10, 1, 5)])
POSE_SCRIPT = {
    (0, 0): 0,      # add into an empty slot
    (0, 4): 3,      # the occupant (point 8, three observations) has more: point 4 is replaced by it
    (0, 5): 4,      # the occupant (point 9, two) has no more than point 5 (two): point 9 is replaced by point 5 -- also in key frame 2
    (0, 6): 5,      # the occupant is bad: nothing happens, and it counts
    (0, 7): 1, (0, 11): 1,   # two points take slot 1: the first is added, the second finds it there and is replaced by it
    (1, 4): 0,      # point 4 was made bad by target 0: skipped
    (1, 5): 0,      # point 5 entered key frame 2 through target 0's Replace: skipped
    (1, 7): 2,      # point 7 survived a Replace: stale, and added
    (1, 0): 1,      # the other direction once more: point 0 (two observations by now) is replaced by point 8 (four)
    (2, 6): 2,      # add
    (2, 0): 3,      # point 0 is bad by now: skipped
}


def test_the_pose_overload_gathers_once_and_replays_in_order():
    answers, per_target = scripted(POSE, POSE_SCRIPT)
    res, calls, _ = run(POSE, answers)
    assert res["status"] == [0] and len(calls) == 1              # one library call
    m, pts = model_of(POSE)
    fused, n_stale, lists = fo.fuse_pose_model(m, POSE["targets"], pts, per_target)
    check_gathered(POSE, calls[0], lists)
    # the lists: non-null, not bad, not in the target
    assert all(2 not in l and 3 not in l and 10 not in l for l in lists) and 1 not in lists[0] and 1 in lists[1] and 5 not in lists[2]
    assert res["fused"] == fused == [6, 2, 1] and res["stale"] == [n_stale] and n_stale == 2     # point 7 in targets 1 and 2
    map_equals(res, m, pts)
    st = m.state()
    assert st["bad"][4] and st["bad"][9] and st["bad"][11] and st["bad"][0] and not st["bad"][8] and not st["bad"][5]
    assert st["slots"][1][4] == 5 and st["slots"][2][6] == 5 and st["slots"][1][1] == 7 and st["slots"][2][2] == 7 and st["slots"][3][2] == 6
    assert st["obs"][8] == {1: 3, 2: 1, 3: 0, 0: 2} and st["slots"][1][0] is None       # point 0 died: its slots went to point 8 or were emptied


SIM3 = dict(mode="sim3", th=4.0, callback=1, kfs=[8, 6, 8, 5], points=[0, 0, None, 1, 0, 0, 0, 0, 0, 0, 1, 0], targets=[1, 2],
            obs=[(0, 0, 0), (1, 0, 1), (4, 0, 2), (5, 0, 3), (6, 0, 4), (8, 1, 3), (8, 2, 1), (8, 3, 0), (9, 2, 6), (10, 1, 5), (11, 1, 2)])
SIM3_SCRIPT = {
    (0, 0): 3,      # occupied by point 8: named as its replacement; the callback lets point 0 take over point 8's slots, key frame 2's too
    (0, 4): 0,      # add
    (0, 6): 5,      # the occupant is bad: nothing, and it counts
    (0, 5): 2,      # occupied by point 11 (seen in key frame 1 only): named; point 5 survives the callback's Replace
    (1, 0): 0,      # point 0 is in key frame 2 by now: skipped
    (1, 4): 6,      # occupied by point 9: named
    (1, 5): 0,      # stale, and added
}


def test_the_sim3_overload_fills_the_replacements_and_sees_the_callback():
    answers, per_target = scripted(SIM3, SIM3_SCRIPT)
    res, calls, _ = run(SIM3, answers)
    assert res["status"] == [0] and len(calls) == 1 and res["called"] == [0, 1]
    m, pts = model_of(SIM3)
    fused, n_stale, lists, replace = fo.fuse_sim3_model(m, SIM3["targets"], pts, per_target)
    check_gathered(SIM3, calls[0], lists)
    assert res["fused"] == fused == [4, 2] and res["stale"] == [n_stale] and n_stale == 1
    assert res["replace"] == replace and replace[0][0] == 8 and replace[0][5] == 11 and replace[1][4] == 9 and replace[1][0] is None
    assert all(len(r) == len(pts) for r in res["replace"])
    map_equals(res, m, pts)
    # without the callback the map the second target sees is another one: point 0 is not in key frame 2 and finds slot 0 empty
    plain = dict(SIM3, callback=0)
    res2, _, _ = run(plain, answers)
    m2, _ = model_of(plain)
    fused2, n_stale2, _, replace2 = fo.fuse_sim3_model(m2, plain["targets"], pts, per_target, apply_replacements=False)
    assert res2["fused"] == fused2 == [4, 3] and res2["replace"] == replace2 and res2["called"] == [0, 1]
    map_equals(res2, m2, pts)


def test_a_failed_call_leaves_map_and_outputs_untouched():
    for scene, script in ((POSE, POSE_SCRIPT), (SIM3, SIM3_SCRIPT)):
        answers, _ = scripted(scene, script)
        res, calls, err = run(scene, answers, QSP_STUB_FAIL="fuse")
        assert res["status"] == [3] and calls == [] and res["fused"] == [-4] and res["stale"] == [-5] and res["replace"] == [[None]] and res["called"] == []
        assert "qsp_fuse_batch failed" in err
        m, pts = model_of(scene)
        map_equals(res, m, pts)


def test_no_target_makes_no_call():
    res, calls, _ = run(dict(POSE, targets=[]), {})
    assert res["status"] == [0] and calls == [] and res["fused"] == [] and res["stale"] == [0]
