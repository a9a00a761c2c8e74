"""CPU: the two restatements of tests/place_db_oracle.py against each other and against the reference's own numbers.

`Literal` walks an inverted file as KeyFrameDatabase does; `Flat` has none and orders the sharing key frames by (first common
word, list sequence number), which is what the device does.  They must give the same taps, candidates and order on every scene and
on 200 seeded random histories: that is the proof that the key order equals the list walk.  The L1 score of `Literal` must equal,
bit for bit, the doubles the reference's L1Scoring::score returned (tests/golden/place_l1_scores.npz, tools/gen_golden_place.py)."""
import os

import numpy as np
import pytest

from tests import place_db_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "place_l1_scores.npz")


def both(ops):
    return po.run_history(po.Literal(), ops), po.run_history(po.Flat(), ops)


@pytest.mark.parametrize("name", sorted(po.scenes()))
def test_literal_and_flat_agree_on_every_scene(name):
    lit, flat = both(po.scenes()[name])
    assert len(lit) == len(flat) > 0
    for a, b in zip(lit, flat):
        assert po.differing(b, a) == 0


@pytest.mark.parametrize("n", po.LARGE_SIZES)
def test_literal_and_flat_agree_on_the_large_scenes(n):
    lit, flat = both(po.large_scene(n))
    assert sum(po.differing(b, a) for a, b in zip(lit, flat)) == 0
    assert [a["n_sharing"] for a in lit] == [n, n - 2, n, n - 1] and len(lit[2]["acc_score"]) == n


def test_literal_and_flat_agree_on_200_random_histories():
    n_query = n_sharing = n_cand = n_tied = 0
    for seed in range(200):
        lit, flat = both(po.random_history(seed))
        for a, b in zip(lit, flat):
            assert po.differing(b, a) == 0, seed
            n_query += 1
            n_sharing += a["n_sharing"]
            n_cand += len(a["cand_id"])
            n_tied += len(a["sharing_first"]) - len(set(a["sharing_first"].tolist()))
    assert n_query > 800 and n_sharing > 5000 and n_cand > 500 and n_tied > 2000      # the histories do have work and ties in them


def test_the_scenes_do_what_they_are_named_for():
    S = po.scenes()
    lit = {k: po.run_history(po.Literal(), v) for k, v in S.items()}
    for m, t in ((5, 4), (10, 8), (15, 12)):
        for r in lit["truncation_max_common_%d" % m]:
            assert (r["max_common"], r["min_common"]) == (m, t)
            assert list(r["sharing_id"]) == [1, 2, 3, 4] and list(r["sharing_common"]) == [t, m, t + 1, t - 1]
            assert list(r["match_id"]) == [2, 3]                      # the one AT minCommonWords is not scored
    r = lit["score_equal_to_min_score_is_kept"]
    assert list(r[0]["match_id"]) == [1, 2, 4] and r[0]["match_score"][1] == po.f32(0.25) == r[0]["min_score_used"]
    assert list(r[1]["match_id"]) == [1, 2, 4] and r[1]["min_score_used"] == po.f32(0.25)
    for r in lit["acc_equal_to_retain_is_dropped"]:
        assert list(r["match_id"]) == [1, 2, 3] and r["acc_score"][1] == po.f32(0.75) * r["acc_score"][0]
        assert list(r["cand_id"]) == [1, 3]
    for r in lit["two_entries_one_best"]:
        assert list(r["best_id"]) == [3, 3, 3] and list(r["cand_id"]) == [3]
    for r in lit["list_order_is_not_id_order"]:
        assert list(r["sharing_id"][:3]) == [9, 3, 7]
    r = lit["unlisted_ref_then_listed"]
    assert 50 not in r[0]["sharing_id"] and 50 not in r[1]["sharing_id"] and 50 in r[2]["sharing_id"] and 50 in r[3]["sharing_id"]
    assert r[0]["min_score_used"] == po.f32(1.0) or r[0]["min_score_used"] < 1            # the unlisted ref was scored
    r = lit["ref_without_common_word"]
    assert r[0]["min_score_used"] == 0 and np.signbit(r[0]["min_score_used"])             # -0.0f: every scored key frame passes
    assert len(r[0]["match_id"]) > 0 and r[1]["min_score_used"] == 0
    r = lit["all_excluded"]
    assert r[0]["n_sharing"] == 0 and r[1]["n_sharing"] <= 1
    r = lit["wave_edges_63_64_65_4097"]
    assert all(x["n_sharing"] >= 4 for x in r[:2]) and max(x["max_common"] for x in r) > 2000
    r = lit["empty_query"]
    assert all(x["n_sharing"] == 0 for x in r) and r[2]["min_score_used"] == 0


def test_the_stale_reloc_score_scene():
    """query 2 stamps B without scoring it; as A's neighbour B adds the score that query 1 left (:273-281)"""
    r = po.run_history(po.Literal(), po.stale_reloc_scene())
    q1, q2, l1, l2 = r
    assert list(q1["match_id"]) == [2] and q1["match_score"][0] > 0
    assert list(q2["sharing_id"]) == [1, 2] and list(q2["sharing_common"]) == [20, 1] and list(q2["match_id"]) == [1]
    assert q2["acc_score"][0] == po.f32(q2["match_score"][0] + q1["match_score"][0])      # B's score from query 1
    # the loop pass reads a neighbour's score only when this query scored it
    assert list(l2["match_id"]) == [1] and l2["acc_score"][0] == l2["match_score"][0]


def test_l1_score_equals_the_references_bit_for_bit():
    z = np.load(GOLDEN)
    off, word, value, want = z["off"], z["word"], z["num"].astype(np.float64) / float(1 << 20), z["score"]
    assert len(want) >= 200
    lens = set()
    n_bad = 0
    for (a, b, c), s in zip(off, want):
        v1 = (word[a:b].tolist(), value[a:b].tolist())
        v2 = (word[b:c].tolist(), value[b:c].tolist())
        lens.update((b - a, c - b))
        if b > a:
            assert abs(sum(v1[1]) - 1) < 1e-12 and min(v1[1]) > 0
        n_bad += np.float64(po.l1_score(v1, v2)).view(np.uint64) != np.float64(s).view(np.uint64)
    assert lens == {0, 1, 63, 64, 65, 1500}
    assert n_bad == 0
    assert want.max() == 1.0 and (want == 0).sum() > 20 and ((want > 0) & (want < 1)).sum() > 40
