"""GPU: the one-shot batch calls share one cache of device blocks (csrc/staging.hpp, csrc/buf_cache.hpp), so a call may be handed
the block another call has just filled.  No call may depend on what that block held.

Small seeded fixtures of the existing oracle modules (2 candidates or objects, one of them empty, the tap outputs requested): every
block but the essential graph's is under 64 KiB, so by the cache's best-fit rule (asked <= have <= 2 x asked + 64 KiB) these calls
recycle each other's blocks.  The essential graph's block cannot be that small (H, A and Uf padded to the factorisation's 64-wide
block, W and J: about 480 KiB for the 10 free key frames here) and none of the small calls can hand it one.  Its two entry points
are therefore neighbours in ORDER_2 -- the stages call (no map points, the smaller block) inherits the block of the optimisation --
and the optimisation also runs behind itself on the same graph with every map point twice: a block a few KiB larger, inside the
window, in which every array behind the points (the states, E, J, b, x, W, H, A, Uf) lay at other offsets.

Round 1 runs every call on fresh memory (release_caches before each) and must equal the oracles at the bars of each entry point's
own suite.  Round 2 runs every call straight after another one, with the cache emptied first, so that the cache holds exactly the
block that other call has just filled; the call inherits it when it is at least as large as its own.  Both directions of every
neighbouring pair of ORDER_2 are run, so of each pair the smaller call inherits the larger one's block (which call that is, is not
observed: the test asserts results only).  Round 3 is fresh memory again.  Every output array of rounds 2 and 3 must have the
bytes of round 1."""
import json

import numpy as np
import pytest

from tests import essential_oracle as eo
from tests import object_gate_cases as GC
from tests import object_gate_oracle as GO
from tests import search_bow_oracle as bo
from tests import search_sim3_oracle as ss
from tests import sim3_oracle as so
from tests import sim3_ransac_oracle as ro

pytestmark = pytest.mark.gpu

ULP = float(np.finfo(np.float32).eps)
FIX = 0                      # fix_scale of the two Sim3 fixtures
I_OPT = (0, 5)               # tests/sim3_oracle.py POOL[FIX]: the empty candidate and 20 noisy matches
I_RANSAC = (0, 5)            # tests/sim3_ransac_oracle.py POOL: the empty candidate and 63 matches, 142 hypotheses
I_SEARCH = (0, 2)            # tests/search_sim3_oracle.py POOL: n2 = 0 and n2 = 63
EG = "free10"


# ---- one runner per entry point: () -> {name: array}, every output of the call ----------------------------------------------
def _flat(results, keys):
    return {"%d/%s" % (i, k): np.asarray(r[k]) for i, r in enumerate(results) for k in keys}


def _bow_fixture(name):
    shared, pool, sis = bo.scenes()[name]
    empty = bo.make_frame(np.zeros((0, 32), np.uint8), [], [])
    return shared, [pool[7], empty, pool[4]], sis, bo.params_of(name)[0]      # 64 or 63 and 100 or 120 key points


def run_bow(name):
    from qsp_slam_amd.ba import search_by_bow_batch
    shared, cands, sis, p = _bow_fixture(name)
    return _flat(search_by_bow_batch(shared, cands, shared_is_source=sis, check_orientation=True, tap=True, **p), bo.KEYS + ("n_matches",))


def run_search_sim3():
    from qsp_slam_amd.ba import search_by_sim3_batch
    res = search_by_sim3_batch(ss.key_frame_1(), [ss.pool()[i] for i in I_SEARCH], tap=True)
    return _flat(res, ("match12", "best1", "dist1", "best2", "dist2", "n_found"))


def run_ransac():
    from qsp_slam_amd.ba import sim3_ransac_batch
    res = sim3_ransac_batch([ro.pool(FIX)[i] for i in I_RANSAC], ro.MIN_INLIERS, bool(FIX), counts=True)
    return _flat(res, ("first_it", "R", "t", "s", "inlier", "n_inliers", "hyp_inliers"))


def run_sim3_opt():
    from qsp_slam_amd.ba import optimize_sim3_batch
    res = optimize_sim3_batch([so.pool(FIX)[i] for i in I_OPT], so.TH2, FIX, trace=True)
    return _flat(res, ("sim3", "inlier", "n_inliers", "iters", "trace"))


def run_essential(copies=1):
    """copies = 2: the same graph with every map point twice, so a block a few KiB larger with every array behind P elsewhere"""
    from qsp_slam_amd.ba import essential_graph_optimize
    sc = eo.fixture(EG)
    g = essential_graph_optimize(sc["sim3"], sc["fixed"], sc["v0"], sc["v1"], sc["meas"], fix_scale=sc["fix_scale"], n_iter=sc["n_iter"],
                                 lambda_init=sc["lambda_init"], pts=np.tile(sc["pts"], (copies, 1)), pt_ref=np.tile(sc["ref"], copies))
    return {k: np.asarray(g[k]) for k in ("sim3", "pts", "iters", "trace")}


def run_essential_stages():
    from qsp_slam_amd.ba import essential_graph_stages
    sc = eo.fixture(EG)
    g = essential_graph_stages(sc["sim3"], sc["fixed"], sc["v0"], sc["v1"], sc["meas"], sc["fix_scale"], 1e-3)
    return {k: np.asarray(v) for k, v in g.items()}


def _gate_cases():
    p, m = GC.pca_cases(), GC.model_cases()
    return [dict(p["n19"]), dict(p["n0_empty"]), {k: m["verts11"][k] for k in ("pts_world", "vertices", "T_wo")}]


def run_gate():
    from qsp_slam_amd import gate_object_points
    out = {}
    for i, g in enumerate(gate_object_points(_gate_cases())):
        out.update({"%d/%s" % (i, k): np.asarray(v) for k, v in
                    dict(erased=g.erased, outlier=g.outlier, whl=[g.w, g.h, g.l], R=g.R, centre_w=g.centre_w, T_wo=g.T_wo, status=g.status).items()
                    if v is not None})                           # (a mesh-gated object has no PCA pose)
    return out


def _planes_fixture():
    from tests.test_gpu_ellipsoid import _scene
    return _scene(np.random.default_rng(5), 2, [9, 0], noise=0.01)[:2]


def run_ell_planes():
    from qsp_slam_amd.ellipsoid import optimize_ellipsoids_using_planes
    ells, planes = _planes_fixture()
    return dict(zip(("ell", "chi2", "iters", "trace"), map(np.asarray, optimize_ellipsoids_using_planes(ells, planes, 10, trace=True))))


def _prior_fixture():
    from oracle import ellipsoid_oracle as EO
    from tests.test_oracle_ellipsoid import _prior_scene
    rng = np.random.default_rng(21)
    scenes = [_prior_scene(rng, yaw_err=rng.uniform(-0.15, 0.15)) for _ in range(2)]
    return dict(ells=np.array([s[1] for s in scenes]), pn=[s[2] for s in scenes], pl=[s[3] for s in scenes],
                pri=np.array([EO.pri_of(s[0][7:]) for s in scenes]), w=np.array([0.8, 1.6]), gw=np.array([1.5, 2.5]))


def run_ell_prior():
    from qsp_slam_amd.ellipsoid import infer_ellipsoids_with_prior
    f = _prior_fixture()
    res = infer_ellipsoids_with_prior(f["ells"], f["pn"], f["pl"], f["pri"], f["w"], angle_sigma_deg=10.0, ground_plane_weight=f["gw"], trace=True)
    return dict(zip(("ell", "chi2", "iters", "trace"), map(np.asarray, res)))


RUNNERS = dict(bow_kf=lambda: run_bow("kf_pool"), bow_frame=lambda: run_bow("frame_pool"), search_sim3=run_search_sim3, ransac=run_ransac,
               sim3_opt=run_sim3_opt, essential=run_essential, essential_stages=run_essential_stages, gate=run_gate,
               ell_planes=run_ell_planes, ell_prior=run_ell_prior)
ORDER_2 = ("gate", "ransac", "bow_frame", "ell_prior", "sim3_opt", "search_sim3", "essential", "essential_stages", "ell_planes", "bow_kf")
PREDECESSORS = dict(essential_more_points=lambda: run_essential(copies=2))       # run only to leave their block behind
EXTRA_PAIRS = (("essential_more_points", "essential"),)


# ---- round 1 against the oracles, at the bars of each entry point's own suite -------------------------------------------------
def check_bow(got, name):
    shared, cands, sis, p = _bow_fixture(name)
    for i, c in enumerate(cands):
        if len(c["angle"]) == 0 and not sis:
            assert got["%d/n_matches" % i] == 0 and len(got["%d/match" % i]) == 0
            continue
        want = bo.literal(shared, c, shared_is_source=sis, check_orientation=True, **p)
        for k in bo.KEYS + ("n_matches",):                       # test_gpu_search_bow: no tolerance
            assert np.array_equal(got["%d/%s" % (i, k)], want[k]), (name, i, k)


def check_search_sim3(got):
    width = ss.band()                                            # test_gpu_search_sim3: a slot may differ only inside the band
    for k, i in enumerate(I_SEARCH):
        r = ss.search(ss.key_frame_1(), ss.pool()[i], "f64")
        for d in (1, 2):
            diff = (got["%d/best%d" % (k, d)] != r["best%d" % d]) | (got["%d/dist%d" % (k, d)] != r["dist%d" % d])
            assert not diff.any() or float(r["knife%d" % d][diff].max()) < width, (i, d)
        sure = r["knife1"] >= width
        j = r["best1"]
        if len(r["knife2"]):
            sure &= np.where(j >= 0, r["knife2"][np.maximum(j, 0)] >= width, True)
        assert np.array_equal(got["%d/match12" % k][sure], r["match12"][sure]), i
        assert got["%d/n_found" % k] == int((got["%d/match12" % k] >= 0).sum())


def check_ransac(got):
    for k, i in enumerate(I_RANSAC):                             # test_gpu_sim3_ransac.test_first_success_and_transform
        c, r = ro.pool(FIX)[i], ro.evaluate(ro.pool(FIX)[i], FIX, "f64")
        first = ro.first_success(r["count"], c["n_its"])
        assert got["%d/first_it" % k] == first, (i, got["%d/first_it" % k], first)
        assert got["%d/n_inliers" % k] == int(got["%d/inlier" % k].sum())
        if not first:
            assert not got["%d/R" % k].any() and not got["%d/t" % k].any() and got["%d/s" % k] == 0
            continue
        h = first - 1
        dist = ro.flavour_distance(FIX, i, h)
        scale = dict(R=1.0, t=max(1.0, float(np.abs(r["t"][h]).max())), s=max(1.0, float(r["s"][h])))
        for q in ("R", "t", "s"):
            err = float(np.abs(got["%d/%s" % (k, q)].astype(np.float64) - r[q][h]).max())
            assert err <= max(4 * dist[q], 4 * ULP * scale[q]), (i, q, err)


def check_sim3_opt(got):
    bar = json.load(open(so.MARGINS))["bar"]                     # test_gpu_sim3.test_batch_of_17_against_the_oracle
    for k, i in enumerate(I_OPT):
        r = so.optimize_sim3(so.pool(FIX)[i], so.TH2, FIX)
        g = {q: got["%d/%s" % (k, q)] for q in ("sim3", "inlier", "n_inliers", "iters", "trace")}
        assert np.array_equal(g["inlier"], r["inlier"]) and g["n_inliers"] == r["n_inliers"] and list(g["iters"]) == list(r["iters"]), i
        assert np.array_equal(g["trace"][:, :, 2], r["trace"][:, :, 2]), i
        d = so.sensitivity(g, r)
        assert all(d[q] <= bar[q] for q in d), (i, d, bar)


def check_essential(got):
    r = eo.fixture_result(EG)                                    # test_gpu_essential.test_against_the_oracle
    g = dict(got, iters=int(got["iters"]))
    assert g["iters"] == r["iters"]
    assert [[False] * (int(t[2]) - 1) + [bool(t[3])] for t in g["trace"]] == r["accepts"]
    d, bar = eo.distance(g, r), eo.bars(EG)
    assert all(d[k] <= bar[k] for k in d), (d, bar)


def check_gate(got):
    for i, c in enumerate(_gate_cases()):                        # test_gpu_object_gate._check_flags
        ref = GO.gate(c, "f64")
        keep = ref["edge"] >= GC.BAND
        assert got["%d/status" % i] == ref["status"], i
        assert np.array_equal(got["%d/erased" % i][keep], ref["erased"][keep]) and np.array_equal(got["%d/outlier" % i][keep], ref["outlier"][keep]), i


def check_ell(got, fit_of, n_checked):
    for i in range(n_checked):                                   # test_gpu_ellipsoid: ellipsoid 1e-5, chi2 1e-6 relative
        r = fit_of(i)
        assert np.abs(got["ell"][i] - r["ell"]).max() < 1e-5
        assert abs(got["chi2"][i] - r["chi2"]) < 1e-6 * max(1.0, r["chi2"]) + 1e-9


def check_round_1(first):
    from oracle import ellipsoid_oracle as EO
    check_bow(first["bow_kf"], "kf_pool")
    check_bow(first["bow_frame"], "frame_pool")
    check_search_sim3(first["search_sim3"])
    check_ransac(first["ransac"])
    check_sim3_opt(first["sim3_opt"])
    check_essential(first["essential"])
    check_gate(first["gate"])
    ells, planes = _planes_fixture()
    check_ell(first["ell_planes"], lambda i: EO.fit(ells[i], planes[i], 10, False), 1)       # (no plane: nothing determined)
    f = _prior_fixture()
    check_ell(first["ell_prior"], lambda i: EO.prior_fit(f["ells"][i], f["pn"][i], f["pl"][i], f["pri"][i], f["w"][i], 10.0, f["gw"][i]), 2)


def same_bits(a, b):
    """the names of the outputs whose bytes differ (bit identity: -0.0 is not 0.0, a NaN equals only its own payload)"""
    assert a.keys() == b.keys()
    return [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]


def test_no_call_depends_on_what_a_recycled_block_held():
    from qsp_slam_amd.ba import release_caches

    def fresh(name):
        release_caches()
        return RUNNERS[name]()

    def after(prev, name):                                       # the cache holds exactly the block `prev` has just filled
        release_caches()
        (RUNNERS.get(prev) or PREDECESSORS[prev])()
        return RUNNERS[name]()

    first = {name: fresh(name) for name in RUNNERS}
    check_round_1(first)
    assert set(ORDER_2) == set(RUNNERS) and tuple(RUNNERS) != ORDER_2
    for i, name in enumerate(ORDER_2):                           # behind both neighbours: of each pair the smaller inherits
        for prev in (ORDER_2[i - 1], ORDER_2[(i + 1) % len(ORDER_2)]):
            assert same_bits(after(prev, name), first[name]) == [], (prev, name)
    for prev, name in EXTRA_PAIRS:
        assert same_bits(after(prev, name), first[name]) == [], (prev, name)
    for name in RUNNERS:
        assert same_bits(fresh(name), first[name]) == [], name
