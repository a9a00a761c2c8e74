"""CPU: the relocalisation and Sim3 overloads of OrbMatcherHip::SearchByProjection (include/qsp_optimizer_shim.h), compiled against
the stand-in frame, key frame and point of tests/shim_mock_projection_kf/ and a stub of qsp_search_by_projection_kf that records what
it is given and answers from a script.  A stand-alone program (sanitised), never loaded into Python.  Every gathered value is
restated here in float32 from the procedural scene of projection_kf_caller.cpp; a non-null slot whose point has ZERO observations
must be gathered as taken; the write-back is checked against the scripted answers; a failed status must write nothing."""
import os
import subprocess
import tempfile

import numpy as np

from tests import search_projection_kf_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_mock_projection_kf")
_EXE = {}
f32 = np.float32
INTS = ("octave", "desc", "slot_blocked", "src_valid", "src_desc")


def build():
    if "exe" in _EXE:
        return _EXE["exe"]
    tmp = tempfile.mkdtemp(prefix="qsp_shim_projection_kf_")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    inc = ["-I" + MOCK, "-I" + os.path.join(ROOT, "include")]
    o = lambda n: os.path.join(tmp, n)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DQSP_SHIM_MOCK_TYPES=1"] + san + inc + ["-c", os.path.join(MOCK, "projection_kf_caller.cpp"), "-o", o("caller.o")])
    subprocess.check_call(["gcc", "-std=c11", "-O1"] + san + ["-I" + os.path.join(ROOT, "include"), "-c", os.path.join(MOCK, "stub_projection_kf.c"), "-o", o("stub.o")])
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
                    calls.append(dict(zip(("mode", "n_src", "n", "check_orientation", "orb_dist"), map(int, v))))
                elif k == "frame":
                    calls[-1].update(zip(("cols", "rows", "n_levels"), map(int, v)))
                else:
                    calls[-1][k] = np.array(v, np.int64 if k in INTS else f32)
    res = {}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        res[k] = [int(x) for x in v] if k == "slots" else int(v[0])
    return res, calls, r.stderr


# ---- the procedural scene of projection_kf_caller.cpp, restated in float32 ---------------------------------------------------------
def frame(k, n):
    k_, j = f32(k), np.arange(n, dtype=f32)
    min_x, max_x, min_y, max_y = f32(-1.5) - k_, f32(640.5) + k_, f32(-2.25), f32(481.75)
    T = np.array([[(f32(0.9) if r == c else f32(0.1) * f32(r - c)) + f32(0.01) * k_ for c in range(3)] for r in range(3)], f32)
    return dict(grid=(64, 48, 4), geom=np.array([min_x, max_x, min_y, max_y, f32(64) / (max_x - min_x), f32(48) / (max_y - min_y), f32(0.2) + f32(0.01) * k_], f32),
                sf=np.array([f32(1) + f32(0.25) * f32(l) + f32(0.01) * k_ for l in range(4)], f32), Rcw=T.reshape(-1),
                tcw=np.array([f32(0.3) * f32(r) - f32(0.2) * k_ + f32(1.7) for r in range(3)], f32),
                kp=np.stack([f32(1.5) * j + k_, f32(2.25) * j - k_], -1).astype(f32).reshape(-1), octave=(np.arange(n) + k) % 4,
                angle=(f32(10) * j + k_).astype(f32),
                desc=np.array([[(jj * 7 + b * 3 + k) & 255 for b in range(32)] for jj in range(n)], np.int64).reshape(-1),
                K=np.array([f32(500) + k_, f32(510) + k_, f32(320) + f32(0.5) * k_, f32(240) - f32(0.25) * k_], f32))


def key_frame(k, n):
    k_, j = f32(k), np.arange(n, dtype=f32)
    min_x, max_x, min_y, max_y = f32(-3 - k), f32(650 + k), f32(-4), f32(490)
    cols, rows = 60 + k, 40 + k
    return dict(grid=(cols, rows, 5), geom=np.array([min_x, max_x, min_y, max_y, f32(cols) / (max_x - min_x), f32(rows) / (max_y - min_y), f32(0.3) + f32(0.01) * k_], f32),
                sf=np.array([f32(1) + f32(0.5) * f32(l) + f32(0.01) * k_ for l in range(5)], f32),
                kp=np.stack([f32(2.5) * j + k_, f32(3.25) * j - k_], -1).astype(f32).reshape(-1), octave=(np.arange(n) + k) % 5,
                angle=(f32(7) * j + k_).astype(f32),
                desc=np.array([[(jj * 11 + b * 5 + k) & 255 for b in range(32)] for jj in range(n)], np.int64).reshape(-1),
                K=np.array([f32(400) + k_, f32(410) + k_, f32(300) + f32(0.5) * k_, f32(200) - f32(0.25) * k_], f32))


def point(i):
    i_ = f32(i)
    dmaxi = f32(1.2) * (f32(10) + i_)
    return dict(Xw=np.array([f32(0.1) * i_ + f32(1), f32(0.2) * i_ - f32(1), f32(0.05) * i_ + f32(3)], f32),
                normal=np.array([f32(0.01) * i_, f32(0.02) * i_, f32(1) - f32(0.001) * i_], f32), dist_min_inv=f32(0.8) * (f32(1) + f32(0.1) * i_),
                dist_max_inv=dmaxi, dist_max=dmaxi / f32(1.2), src_desc=np.array([(i * 5 + b) & 255 for b in range(32)], np.int64))


def check_frame(c, F, th):
    assert (c["n"], c["cols"], c["rows"], c["n_levels"]) == (7,) + F["grid"]
    assert np.array_equal(c["geom"], np.append(F["geom"], f32(th)))
    for key in ("sf", "kp", "octave", "desc", "K"):
        assert np.array_equal(c[key], F[key]), key
    assert list(c["slot_blocked"]) == [0, 0, 1, 0, 1, 0, 0]            # slot 4 holds a point with ZERO observations: taken all the same


def check_sources(c, valid, keys):
    assert list(c["src_valid"]) == valid
    for i, ok in enumerate(valid):
        if not ok:
            continue
        P = point(i)
        for key in ("Xw", "src_desc", "dist_min_inv", "dist_max_inv", "dist_max") + keys:
            w = np.size(P[key])
            assert np.array_equal(c[key][w * i:w * i + w], np.reshape(P[key], -1)), (key, i)


def test_the_relocalisation_overload_gathers_every_value_and_writes_back():
    res, calls, _ = run("reloc", "slot 0 4\nslot 2 -2\nslot 5 0\nn_matches 2\n")
    assert res["status"] == 0 and len(calls) == 1
    c, F, KF = calls[0], frame(1, 7), key_frame(2, 6)
    assert (c["mode"], c["n_src"], c["check_orientation"], c["orb_dist"]) == (0, 6, 1, 100)
    check_frame(c, F, 10.0)
    assert np.array_equal(c["Rcw"], F["Rcw"]) and np.array_equal(c["tcw"], F["tcw"])
    assert np.array_equal(c["Ow"], -ko._rowdot(F["Rcw"].reshape(3, 3).T.copy(), F["tcw"], f32))   # -Rcw.t() * tcw
    assert np.array_equal(c["kp_angle"], F["angle"])
    valid = [1, 0, 0, 0, 1, 1]                                         # 1 null, 2 bad, 3 in sAlreadyFound
    check_sources(c, valid, ())
    assert len(c["normal"]) == 0                                       # not gathered: RELOC has no angle test
    for i, ok in enumerate(valid):
        if ok:
            assert c["src_angle"][i] == KF["angle"][i], i
    # the write-back: the key frame's points by slot_src, NULL where nulled (the slot that held a point), the rest as it was
    assert res["slots"] == [4, -1, -1, -1, 101, 0, -1] and res["n_matches"] == 2


def test_the_sim3_overload_decomposes_scw_and_writes_back():
    res, calls, _ = run("sim3", "slot 0 5\nslot 6 0\nn_matches 2\n")
    assert res["status"] == 0 and len(calls) == 1
    c, KF = calls[0], key_frame(1, 7)
    assert (c["mode"], c["n_src"], c["check_orientation"], c["orb_dist"]) == (1, 6, 0, 50)
    check_frame(c, KF, 10.0)
    S = np.zeros((3, 4), f32)
    for r in range(3):
        for col in range(3):
            S[r, col] = f32(2) * ((f32(0.6) if r == col else f32(0.3) * f32(col - r)) + f32(0.05) * f32(r))
        S[r, 3] = f32(2) * (f32(0.7) * f32(r) - f32(0.4))
    R, t, Ow = ko.decompose_scw(S)
    assert np.array_equal(c["Rcw"], R.reshape(-1)) and np.array_equal(c["tcw"], t) and np.array_equal(c["Ow"], Ow)
    scw = np.sqrt(sum(float(S[0, k]) ** 2 for k in range(3)))
    assert np.abs(R.astype(np.float64) * scw - S[:, :3]).max() < 1e-6 and abs(scw - 2 * np.sqrt(0.6 ** 2 + 0.3 ** 2 + 0.6 ** 2)) < 1e-6
    check_sources(c, [1, 0, 0, 0, 1, 1], ("normal",))                  # 1 null, 2 bad, 3 among vpMatched already
    assert len(c["kp_angle"]) == 0 and len(c["src_angle"]) == 0
    assert res["slots"] == [5, -1, 3, -1, 101, -1, 0] and res["n_matches"] == 2


def test_a_failed_status_writes_nothing():
    for mode, slots in (("reloc", [-1, -1, 100, -1, 101, -1, -1]), ("sim3", [-1, -1, 3, -1, 101, -1, -1])):
        res, calls, err = run(mode, "slot 0 4\nslot 2 -2\nn_matches 2\n", QSP_STUB_FAIL="projection_kf")
        assert res["status"] == 3 and calls == [] and "qsp_search_by_projection_kf" in err
        assert res["slots"] == slots and res["n_matches"] == 0
