"""CPU: the conditions under which tests/test_gpu_search_projection_kf.py may ask for 0 differing outputs -- the serial restatement
of the relocalisation and Sim3 projection searches reaches every branch, every deliberate mistake changes an output of some
fixture, the parallel rounds equal the serial loop with the round counts as constructed, the exact cases decide as stated, no slot
is ever over-written, and no other source sits on a threshold."""
import collections
import json

import numpy as np
import pytest

from tests import search_projection_kf_oracle as ko
from tests import search_projection_oracle as po

MODES = ko.MODES
IDS = ["reloc", "sim3"]


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_every_branch_is_reached(mode):
    total = sum((ko.result(mode, n)["counters"] for n in ko.fixtures(mode)), collections.Counter())
    assert [b for b in ko.BRANCHES[mode] if total[b] == 0] == []


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_every_mistake_changes_an_output(mode):
    """RELOC refusing z < 0; the closed image test for the half-open one and the reverse; level + 1 for level as the window's top and
    the reverse; `<` at the accept threshold; 100 for orb_dist; the right-image test; the ratio test; a source without observations
    not blocking; the angle test with `<=`; the other mode's order of 1 / z and fx; the tie order (cell y, cell x)"""
    for m in ko.MUTANTS_OF[mode]:
        hit = [n for n in ko.fixtures(mode) if ko.n_differing(ko.result(mode, n, m), ko.result(mode, n)) > 0]
        assert hit, m
    assert set(ko.MUTANTS_OF[ko.RELOC]) | set(ko.MUTANTS_OF[ko.SIM3]) == set(ko.MUTANTS) and len(ko.MUTANTS) >= 10


@pytest.mark.parametrize("mode,mutant,case", [(ko.RELOC, "reloc_z_neg", "z_negative"), (ko.RELOC, "image_half_open", "u_eq_max"),
                                              (ko.SIM3, "image_closed", "u_eq_max"), (ko.RELOC, "window_top_level", "octave_level_plus_1"),
                                              (ko.SIM3, "window_top_plus1", "octave_level_plus_1"), (ko.RELOC, "accept_lt", "dist_at_th"),
                                              (ko.SIM3, "accept_lt", "dist_at_th"), (ko.SIM3, "accept_100", "dist_above_th"),
                                              (ko.RELOC, "right_test", "right_far"), (ko.SIM3, "right_test", "right_far"),
                                              (ko.RELOC, "ratio_test", "no_ratio"), (ko.SIM3, "ratio_test", "no_ratio"),
                                              (ko.SIM3, "angle_le", "angle_eq"), (ko.RELOC, "tie_cy_cx", "tie_diag"), (ko.SIM3, "tie_cy_cx", "tie_diag")])
def test_the_mistake_is_caught_by_the_case_made_for_it(mode, mutant, case):
    c = ko.fixtures(mode)["edges"]["cases"][case]
    assert ko.differs(ko.result(mode, "edges", mutant), ko.result(mode, "edges"))[c["src"]].any()


def test_the_remaining_mistakes_are_caught_where_expected():
    # 100 where orb_dist is 64: the key point at 65
    c = ko.fixtures(ko.RELOC)["edges_64"]["cases"]["dist_above_th"]
    assert ko.result(ko.RELOC, "edges_64", "accept_100")["choice"][c["src"][0]] == c["kp"][0] and ko.result(ko.RELOC, "edges_64")["choice"][c["src"][0]] == -1
    for mode in MODES:
        # a source whose point has no observations blocks all the same: the second of the pair must move on
        c = ko.fixtures(mode)["contention"]["cases"]["pair"]
        assert list(ko.result(mode, "contention", "non_blocking")["choice"][c["src"]]) == [c["kp"][0], c["kp"][0]]
        # the order of 1 / z and fx: only the last bit of u and v, which the taps show on the rotated frames
        m = "reloc_invz_order" if mode == ko.RELOC else "sim3_invz_order"
        a, b = ko.result(mode, "random_0", m), ko.result(mode, "random_0")
        assert (a["proj_x"].view(np.uint32) != b["proj_x"].view(np.uint32)).any() or (a["proj_y"].view(np.uint32) != b["proj_y"].view(np.uint32)).any()


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_the_rounds_equal_the_serial_loop(mode):
    for name, f in ko.fixtures(mode).items():
        r, p = ko.result(mode, name), ko.result_rounds(mode, name)
        assert ko.n_differing(p, r) == 0, name
        assert 1 <= p["n_rounds"] <= len(r["choice"]) + 1, name
    for name in ("chain", "contention"):
        assert ko.result_rounds(mode, name)["n_rounds"] == 6, name       # five sources each displacing the next, and the round that repeats
    assert ko.result_rounds(mode, "stride_0")["n_rounds"] == 1           # nothing chosen: round 1 repeats the initial "none"


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_the_named_cases_decide_as_stated(mode):
    seen = set()
    for name in ("contention", "chain", "edges") + (("edges_64", "contention_no_ori") if mode == ko.RELOC else ("scale_half", "scale_two")):
        f, r = ko.fixtures(mode)[name], ko.result(mode, name)
        for case, c in f["cases"].items():
            seen.add(case)
            for key in ("choice", "reason", "dist", "bin", "level"):
                if key in c:
                    assert [int(r[key][i]) for i in c["src"]] == list(c[key]), (name, case, key)
            for slot, who in c.get("slot_src", {}).items():
                assert r["slot_src"][slot] == who, (name, case)
    want = {"pair", "chain", "blocked_initially", "tie_cx", "tie_cy", "tie_cell", "dx_eq_r", "dx_below_r", "dist_at_th", "dist_above_th", "u_eq_min",
            "dist_eq_min_inv", "clamp_0", "clamp_top", "right_far", "z_negative", "z_plus_0", "z_0_x_0", "z_minus_0", "u_eq_max", "u_below_max",
            "octave_level_plus_1", "octave_level_plus_2", "octave_level_minus_2", "angle_eq", "angle_below", "listed_twice"}
    want |= {"bin_wrap", "hist_removed"} if mode == ko.RELOC else set()
    assert want <= seen
    e, r = ko.fixtures(mode)["edges"]["cases"], ko.result(mode, "edges")
    reason = lambda case: int(r["reason"][e[case]["src"][0]])
    if mode == ko.RELOC:
        assert reason("z_negative") == po.MATCHED and reason("z_plus_0") == po.OUTSIDE and reason("z_0_x_0") == po.NONFINITE
        assert reason("u_eq_max") == po.EMPTY                      # inside: searched, nothing there
        assert [ko.fixtures(mode)[n]["opt"]["orb_dist"] for n in ("edges", "edges_64")] == [100, 64]
        assert [ko.fixtures(mode)[n]["cases"]["dist_at_th"]["dist"] for n in ("edges", "edges_64")] == [[100], [64]]
        c = ko.fixtures(mode)["contention"]["cases"]["hist_removed"]
        with_ori, without = ko.result(mode, "contention"), ko.result(mode, "contention_no_ori")
        assert with_ori["slot_src"][c["kp"][0]] == -2 and without["slot_src"][c["kp"][0]] == c["src"][0]
        assert with_ori["n_matches"] == without["n_matches"] - 1 and (without["bin"] == -1).all() and (without["hist"] == 0).all()
    else:
        assert reason("z_negative") == po.Z_NEG and reason("z_minus_0") == po.OUTSIDE          # -0.0 passes the depth test
        assert reason("u_eq_max") == po.OUTSIDE and reason("u_below_max") == po.EMPTY
        assert reason("angle_eq") == po.MATCHED and reason("angle_below") == po.ANGLE
        assert reason("octave_only_outside") == po.NONE_ELIGIBLE
        assert e["dist_at_th"]["dist"] == [50]
        for name, s in (("scale_half", 0.5), ("scale_two", 2.0)):
            f = ko.fixtures(mode)[name]
            assert np.array_equal(f["frame"]["Scw"][:, :3], np.float32(s) * np.asarray(ko.fixtures(mode)["edges"]["frame"]["Rcw"], np.float32))
            assert ko.n_differing(ko.result(mode, name), r) == 0   # the division by scw gives the pose back


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_no_slot_is_over_written(mode):
    for name in ko.fixtures(mode):
        r = ko.result(mode, name)
        taken = r["choice"][r["choice"] >= 0]
        assert len(set(taken.tolist())) == len(taken), name
        removed = int((r["slot_src"] == -2).sum())
        assert r["n_matches"] == len(taken) - removed, name
        assert not np.asarray(ko.fixtures(mode)[name]["frame"]["slot_blocked"], bool)[taken].any(), name
        assert mode == ko.RELOC or removed == 0


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_no_other_source_sits_on_a_threshold(mode):
    smallest, smallest_q = np.inf, np.inf
    for name, f in ko.fixtures(mode).items():
        r = ko.result(mode, name)
        rest = np.array([i not in f["exact"] for i in range(len(r["knife"]))], bool)
        if rest.any():
            smallest = min(smallest, float(np.nanmin(r["knife"][rest])))
            smallest_q = min(smallest_q, float(r["knife_q"][rest].min()))
            assert not np.isnan(r["knife"][rest]).any(), name
    print("%s: smallest knife-edge distance %.3g, of the level decision %.3g" % (IDS[mode], smallest, smallest_q))
    assert smallest > ko.ON_THRESHOLD and smallest_q > ko.THRESHOLD


def test_the_fixture_list():
    for mode in MODES:
        names = set(ko.fixtures(mode))
        assert {"contention", "chain", "edges", "random_0", "random_1", "random_2"} | {"stride_%d" % n for n in (0, 1, 63, 64, 65, 4096, 4097)} <= names
        for n in ko.STRIDE_N:
            assert len(ko.fixtures(mode)["stride_%d" % n]["frame"]["octave"]) == n


def test_the_margins_file_is_all_zeros():
    with open(ko.MARGINS) as fh:
        rec = json.load(fh)
    assert rec and all(k.startswith("search_projection_kf/") and v["measured"] == 0 and v["tol"] == 0 for k, v in rec.items())
    want = {"search_projection_kf/%s/%s/outputs_differing" % (ko.MODE_NAME[m], n) for m in MODES for n in ko.fixtures(m)}
    assert want <= set(rec)


def test_decompose_scw_of_the_package_equals_the_restatement():
    from qsp_slam_amd.ba import decompose_scw
    rng = np.random.default_rng(5)
    for s in (0.5, 2.0, 0.75, 1.3, 3.1):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        S = np.concatenate([s * q, rng.normal(size=(3, 1))], 1).astype(np.float32)
        for a, b in zip(decompose_scw(S), ko.decompose_scw(S)):
            assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    R, t, Ow = decompose_scw(np.array([[2, 0, 0, 4], [0, 2, 0, -6], [0, 0, 2, 8]], np.float32))
    assert np.array_equal(R, np.eye(3, dtype=np.float32)) and list(t) == [2, -3, 4] and list(Ow) == [-2, 3, -4]


def test_the_binding_exports_the_call():
    from qsp_slam_amd import _lib
    assert hasattr(_lib.lib(), "qsp_search_by_projection_kf") and "qsp_search_by_projection_kf" in _lib.SYMBOLS
