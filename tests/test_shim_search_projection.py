"""CPU: OrbMatcherHip::SearchLocalPoints and OrbMatcherHip::SearchByProjection (include/qsp_optimizer_shim.h), compiled against the
stand-in frame and point of tests/shim_mock_projection/ and a stub of qsp_search_by_projection that records what it is given and
answers from a script.  A stand-alone program (sanitised), never loaded into Python.  Every gathered value is restated here in
float32 from the procedural scene of projection_caller.cpp; the write-back is checked against the scripted answers; a failed status
must leave the frame and the points as they were."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_projection")
_EXE = {}
f32 = np.float32
INTS = ("octave", "desc", "slot_blocked", "src_valid", "src_blocks", "src_desc", "src_octave")


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_projection_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc + ["-c", os.path.join(MOCK, "projection_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_projection.c"), "-o", o("stub.o")])
    subprocess.check_call(["g++"] + san + ["-o", o("caller"), o("caller.o"), o("stub.o")])
    _EXE["exe"] = o("caller")
    return _EXE["exe"]


def run(mode, answers="", **env_extra):
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "answers.txt"), "w").write(answers)
        env = {k: v for k, v in os.environ.items() if not k.startswith("QSP_")}
        env.update(QSP_STUB_DUMP=os.path.join(tmp, "dump.txt"), QSP_STUB_ANSWERS=os.path.join(tmp, "answers.txt"), **env_extra)
        r = subprocess.run([build(), mode], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        calls = []
        if os.path.exists(env["QSP_STUB_DUMP"]):
            for line in open(env["QSP_STUB_DUMP"]).read().splitlines():
                k, *v = line.split()
                if k == "call":
                    calls.append(dict(zip(("mode", "n_src", "n", "check_orientation", "mono"), map(int, v))))
                elif k == "frame":
                    calls[-1].update(zip(("cols", "rows", "n_levels", "has_point"), map(int, v)))
                else:
                    calls[-1][k] = np.array(v, np.int64 if k in INTS else f32)
    res = dict(points={})
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "point":
            res["points"][int(v[0])] = dict(in_view=int(v[1]), x=f32(v[2]), y=f32(v[3]), xr=f32(v[4]), level=int(v[5]), cos=f32(v[6]), visible=int(v[7]))
        elif k == "slots":
            res["slots"] = [int(x) for x in v]
        else:
            res[k] = int(v[0])
    return res, calls, r.stderr


# ---- the procedural scene of projection_caller.cpp, restated in float32 ------------------------------------------------------------
def frame(k, n):
    k_, j = f32(k), np.arange(n, dtype=f32)
    min_x, max_x, min_y, max_y = f32(-1.5) - k_, f32(640.5) + k_, f32(-2.25), f32(481.75)
    T = np.array([[(f32(0.9) if r == c else f32(0.1) * f32(r - c)) + f32(0.01) * k_ for c in range(3)] for r in range(3)], f32)
    return dict(geom=np.array([min_x, max_x, min_y, max_y, f32(64) / (max_x - min_x), f32(48) / (max_y - min_y), f32(0.2) + f32(0.01) * k_], f32),
                sf=np.array([f32(1) + f32(0.25) * f32(l) + f32(0.01) * k_ for l in range(4)], f32), Rcw=T.reshape(-1),
                tcw=np.array([f32(0.3) * f32(r) - f32(0.2) * k_ + f32(1.7) for r in range(3)], f32),
                kp=np.stack([f32(1.5) * j + k_, f32(2.25) * j - k_], -1).astype(f32).reshape(-1), octave=(np.arange(n) + k) % 4,
                octave_raw=(np.arange(n) + k + 1) % 4, angle=(f32(10) * j + k_).astype(f32),
                desc=np.array([[(jj * 7 + b * 3 + k) & 255 for b in range(32)] for jj in range(n)], np.int64).reshape(-1),
                K=np.array([f32(500) + k_, f32(510) + k_, f32(320) + f32(0.5) * k_, f32(240) - f32(0.25) * k_, f32(40) + k_], f32),
                Ow=np.array([f32(0.37) * f32(r + 1) - f32(0.11) * k_ for r in range(3)], f32), mb=f32(0.1) + f32(0.01) * k_,
                u_right=np.array([5.0 + jj if jj % 3 == 0 else -1.0 for jj in range(n)], f32))


def point(i):
    i_ = f32(i)
    dmaxi = f32(1.2) * (f32(10) + i_)
    return dict(Xw=np.array([f32(0.1) * i_ + f32(1), f32(0.2) * i_ - f32(1), f32(0.05) * i_ + f32(3)], f32),
                normal=np.array([f32(0.01) * i_, f32(0.02) * i_, f32(1) - f32(0.001) * i_], f32), dist_min_inv=f32(0.8) * (f32(1) + f32(0.1) * i_),
                dist_max_inv=dmaxi, dist_max=dmaxi / f32(1.2), desc=np.array([(i * 5 + b) & 255 for b in range(32)], np.int64), blocks=int(i % 3 > 0))


def check_frame(c, F):
    assert (c["n"], c["cols"], c["rows"], c["n_levels"], c["has_point"]) == (7, 64, 48, 4, 0)
    for key in ("geom", "sf", "Rcw", "tcw", "kp", "octave", "desc", "K", "u_right"):
        assert np.array_equal(c[key], F[key]), key
    assert np.array_equal(c["kp_angle"], F["angle"])
    assert list(c["slot_blocked"]) == [0, 0, 1, 0, 0, 0, 0]            # slot 2 holds an observed point; slot 4 a point without observations


def check_sources(c, valid, keys):
    assert list(c["src_valid"]) == valid
    for i, ok in enumerate(valid):
        if not ok:
            continue
        P = point(i)
        assert c["src_blocks"][i] == P["blocks"], i
        assert np.array_equal(c["Xw"][3 * i:3 * i + 3], P["Xw"]) and np.array_equal(c["src_desc"][32 * i:32 * i + 32], P["desc"]), i
        for key in keys:
            w = np.size(P[key])
            assert np.array_equal(c[key][w * i:w * i + w], np.reshape(P[key], -1)), (key, i)


UNTOUCHED = dict(in_view=0, x=f32(-1), y=f32(-1), xr=f32(-1), level=-1, cos=f32(-1), visible=0)
LOCAL_ANSWERS = "src 0 1 11.5 12.25 3.5 2 0.75\nsrc 4 0 0 0 0 0 0\nsrc 5 1 21.5 22.25 -4.5 0 0.999\nslot 4 5\nslot 6 0\nn_matches 3\n"


def test_search_local_points_gathers_every_value_and_writes_back():
    res, calls, _ = run("local", LOCAL_ANSWERS)
    assert res["status"] == 0 and len(calls) == 1
    c, F = calls[0], frame(1, 7)
    assert (c["mode"], c["n_src"]) == (0, 6)
    check_frame(c, F)
    assert np.array_equal(c["Ow"], F["Ow"]) and np.array_equal(c["opt"][1:], np.array([3.0, 0.8, 0.5], f32))
    check_sources(c, [1, 0, 0, 0, 1, 1], ("normal", "dist_min_inv", "dist_max_inv", "dist_max"))   # 1 null, 2 bad, 3 seen in this frame
    # the write-back: sources only; the projection members and IncreaseVisible only where in view
    p = res["points"]
    assert p[0] == dict(in_view=1, x=f32(11.5), y=f32(12.25), xr=f32(3.5), level=2, cos=f32(0.75), visible=1)
    assert p[5] == dict(in_view=1, x=f32(21.5), y=f32(22.25), xr=f32(-4.5), level=0, cos=f32(0.999), visible=1)
    assert p[4] == UNTOUCHED and p[2] == UNTOUCHED and p[3] == UNTOUCHED
    assert res["slots"] == [-1, -1, 100, -1, 5, -1, 0] and res["n_matches"] == 3


def test_search_by_projection_reads_the_octave_of_mvkeys_and_the_angle_of_mvkeysun():
    res, calls, _ = run("last", "slot 0 3\nslot 2 -2\nslot 4 -2\nslot 5 4\nn_matches 2\n")
    assert res["status"] == 0 and len(calls) == 1
    c, F, L = calls[0], frame(1, 7), frame(2, 6)
    assert (c["mode"], c["n_src"], c["check_orientation"], c["mono"]) == (1, 6, 1, 0)
    check_frame(c, F)
    assert c["opt"][0] == F["mb"] and c["opt"][1] == f32(7.0)
    assert np.array_equal(c["last_Rcw"], L["Rcw"]) and np.array_equal(c["last_tcw"], L["tcw"])
    valid = [1, 0, 0, 1, 1, 1]                                         # 1 null, 2 an outlier; 4 is bad, which the reference does not ask
    check_sources(c, valid, ())
    for i, ok in enumerate(valid):
        if ok:
            assert c["src_octave"][i] == L["octave_raw"][i] != L["octave"][i] and c["src_angle"][i] == L["angle"][i], i
    # the write-back: the last frame's points by slot_src, NULL where nulled (also the slot that held a point), the rest as it was
    assert res["slots"] == [3, -1, -1, -1, -1, 4, -1] and res["n_matches"] == 2
    assert all(v == UNTOUCHED for v in res["points"].values())


def test_a_failed_status_leaves_the_frame_and_the_points_untouched():
    for mode in ("local", "last"):
        res, calls, err = run(mode, LOCAL_ANSWERS, QSP_STUB_FAIL="projection")
        assert res["status"] == 3 and calls == [] and "qsp_search_by_projection" in err
        assert res["slots"] == [-1, -1, 100, -1, 101, -1, -1] and res["n_matches"] == 0
        assert all(v == UNTOUCHED for v in res["points"].values())
