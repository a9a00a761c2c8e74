"""CPU: the conditions under which tests/test_gpu_search_projection.py may ask for 0 differing outputs -- the serial restatement
reaches every branch, every deliberate mistake changes an output of some fixture, the parallel rounds equal the serial loop with
the round counts as constructed, the exact cases decide as stated, and no other source sits on a threshold."""
import collections
import json

import numpy as np
import pytest

from tests import search_projection_oracle as po

MODES = (po.LOCAL, po.LAST)
IDS = ["local", "last"]


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_every_branch_is_reached(mode):
    total = sum((po.result(mode, n)["counters"] for n in po.fixtures(mode)), collections.Counter())
    assert [b for b in po.BRANCHES[mode] if total[b] == 0] == []


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_every_mistake_changes_an_output(mode):
    for m in po.MUTANTS_OF[mode]:
        hit = [n for n in po.fixtures(mode) if not po.same_call(po.result(mode, n), po.result(mode, n, m), mode)]
        assert hit, m
    assert set(po.MUTANTS_OF[po.LOCAL]) | set(po.MUTANTS_OF[po.LAST]) == set(po.MUTANTS)


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_the_rounds_equal_the_serial_loop(mode):
    for name, f in po.fixtures(mode).items():
        r, p = po.result(mode, name), po.result_rounds(mode, name)
        assert po.same_call(r, p, mode), name
        assert 1 <= p["n_rounds"] <= len(r["choice"]) + 1, name
    for name in ("chain", "contention"):
        assert po.result_rounds(mode, name)["n_rounds"] == 6, name       # five sources each displacing the next, and the round that repeats
    assert po.result_rounds(mode, "stride_0")["n_rounds"] == 1           # nothing chosen: round 1 repeats the initial "none"
    assert po.result_rounds(mode, "edges" if mode == po.LOCAL else "edges_neither")["n_rounds"] == 2


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_the_named_cases_decide_as_stated(mode):
    """distance 100 and 101, the ratio at equality, |dx| == radius, u == max_x (inside), z = +0.0 / -0.0, viewCos one float32 step
    either side of the limit and of 0.998, er equal to the radius, and every contention case"""
    seen = set()
    for name in ("contention", "chain", "edges" if mode == po.LOCAL else "edges_neither"):
        f, r = po.fixtures(mode)[name], po.result(mode, name)
        for case, c in f["cases"].items():
            seen.add(case)
            for key in ("choice", "reason", "dist", "dist2", "bin"):
                if key in c:
                    assert [int(r[key][i]) for i in c["src"]] == list(c[key]), (name, case, key)
            for slot, who in c.get("slot_src", {}).items():
                assert r["slot_src"][slot] == who, (name, case)
            if "level" in c:
                assert r["level"][c["src"][0]] == c["level"], case
            if "view_cos" in c and r["in_view"][c["src"][0]]:
                assert r["view_cos"][c["src"][0]] == c["view_cos"], case
    want = {"pair", "chain", "fallback_above", "overwritten", "blocked_initially", "zero_obs_slot", "tie_cx", "tie_cy", "tie_cell", "th_100", "th_101",
            "dx_eq_r", "dx_below_r", "er_eq_r", "er_above_r", "u_eq_max", "u_above_max", "z_plus_0", "z_minus_0", "stereo_mixed"}
    want |= ({"fallback_ratio", "second_blocked", "ratio_eq", "ratio_above", "cos_eq_limit", "cos_below_limit", "cos_above_998", "cos_below_998",
              "clamp_0", "clamp_top"} if mode == po.LOCAL else {"ori_overwritten", "windows", "octave_0", "octave_top", "bin_wrap"})
    assert want <= seen
    r = po.result(mode, "contention")
    c = po.fixtures(mode)["contention"]["cases"]["overwritten"]
    assert r["n_matches"] == int((r["choice"] >= 0).sum()) - (1 if mode == po.LAST else 0)      # both writers counted; LAST: one histogram removal
    assert r["choice"][c["src"][0]] == r["choice"][c["src"][1]] >= 0
    if mode == po.LAST:
        e = po.fixtures(mode)["edges_neither"]["cases"]["windows"]
        for d, want_kp in e["by_direction"].items():
            assert po.result(mode, "edges_" + d)["choice"][e["src"][0]] == want_kp, d
        assert po.result(mode, "edges_mono")["choice"][e["src"][0]] == e["by_direction"]["neither"]
        o = po.fixtures(mode)["contention"]["cases"]["ori_overwritten"]
        assert r["slot_src"][o["kp"][0]] == -2 and list(r["ind"]) == [0, 12, 6] and r["hist"][3] == 1
        assert po.result(mode, "contention_no_ori")["slot_src"][o["kp"][0]] == o["src"][1]


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_no_other_source_sits_on_a_threshold(mode):
    smallest, smallest_q = np.inf, np.inf
    for name, f in po.fixtures(mode).items():
        r = po.result(mode, name)
        rest = np.array([i not in f["exact"] for i in range(len(r["knife"]))], bool)
        if rest.any():
            smallest = min(smallest, float(np.nanmin(r["knife"][rest])))
            smallest_q = min(smallest_q, float(r["knife_q"][rest].min()))
            assert not np.isnan(r["knife"][rest]).any(), name
    print("%s: smallest knife-edge distance %.3g, of the level decision %.3g" % (IDS[mode], smallest, smallest_q))
    assert smallest > po.ON_THRESHOLD and smallest_q > po.THRESHOLD
    with open(po.MARGINS) as fh:
        rec = json.load(fh)
    assert rec and all(k.startswith("search_projection/") and v["measured"] == 0 and v["tol"] == 0 for k, v in rec.items())


def test_the_binding_exports_the_call():
    from qsp_slam_amd import _lib
    assert hasattr(_lib.lib(), "qsp_search_by_projection") and "qsp_search_by_projection" in _lib.SYMBOLS
