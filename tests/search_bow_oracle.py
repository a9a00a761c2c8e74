"""Two numpy restatements of ORBmatcher::SearchByBoW, written independently of each other, and the fixtures of the SearchByBoW tests.

`literal` transcribes the reference loop by loop: the key-frame overload (src/ORBmatcher.cc:522-655) and the frame overload
(:159-288) each in its own function, with the two-iterator walk and lower_bound over the feature vectors, the vbMatched2 /
vpMapPointMatches taken tests, the per-bin index lists and ComputeThreeMaxima (:1601-1642).  `by_sets` intersects the node ids,
takes each source's top-2 with a stable argsort and builds the histogram with np.bincount.  Both use float32 for the five float
operations (the ratio product, the angle difference, the wrap, the product with 1.0f / 30, 0.1f * max1) and round half away
from zero (np.round rounds half to even and is wrong here).

A frame is the dict qsp_slam_amd.ba.search_by_bow_batch takes: desc (n,32) uint8, angle (n,) float32, eligible (n,) uint8 or
None, node_id (ascending), node_off, feat.  Results are indexed by SOURCE slot in both modes: match, match_raw, dist (n_src,),
hist (30,), ind (3,), n_matches.  Where the reference would index with bestIdx == -1 (th = 256 inclusive, no target) both
restatements refuse the match, as the library documents."""
import bisect
import math

import numpy as np

f32 = np.float32
HISTO_LENGTH = 30
FACTOR = f32(1.0) / f32(HISTO_LENGTH)
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(POP[np.bitwise_xor(a, b)].sum())


def rot_bin(a_src, a_tgt):
    rot = f32(a_src) - f32(a_tgt)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    return int(math.floor(float(f32(rot * FACTOR)) + 0.5))      # round(): half away from zero; the value is never below -0.0


def nodes_of(fr):
    """the DBoW2::FeatureVector: ascending list of (node id, [feature indices])"""
    off = np.asarray(fr["node_off"])
    return [(int(i), [int(x) for x in fr["feat"][off[k]:off[k + 1]]]) for k, i in enumerate(np.asarray(fr["node_id"]))]


def _eligible(fr):
    n = len(fr["angle"])
    return np.ones(n, bool) if fr.get("eligible") is None else np.asarray(fr["eligible"]).astype(bool)


def three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _lower_bound(vec, it, key):
    return bisect.bisect_left([v[0] for v in vec], key)


def _result(n_src, match, raw, dist, hist, ind, info):
    return dict(match=np.array(match, np.int32).reshape(n_src), match_raw=np.array(raw, np.int32).reshape(n_src),
                dist=np.array(dist, np.int32).reshape(n_src), hist=np.array(hist, np.int32), ind=np.array(ind, np.int32),
                n_matches=int((np.array(match, np.int32) >= 0).sum()), info=info)


def literal_kf(kf1, kf2, th, th_inclusive, nn_ratio, check_orientation):
    """:522-655; vpMatches12[idx1] holds idx2 in place of the map point"""
    vFeatVec1, vFeatVec2 = nodes_of(kf1), nodes_of(kf2)
    vpMapPoints1, vpMapPoints2 = _eligible(kf1), _eligible(kf2)          # pMP && !pMP->isBad()
    n1 = len(vpMapPoints1)
    vpMatches12 = [-1] * n1
    dist12 = [-1] * n1
    vbMatched2 = [False] * len(vpMapPoints2)
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    info = {}
    f1it, f2it, f1end, f2end = 0, 0, len(vFeatVec1), len(vFeatVec2)
    while f1it != f1end and f2it != f2end:
        if vFeatVec1[f1it][0] == vFeatVec2[f2it][0]:
            for idx1 in vFeatVec1[f1it][1]:
                if not vpMapPoints1[idx1]:
                    continue
                d1 = kf1["desc"][idx1]
                bestDist1, bestIdx2, bestDist2 = 256, -1, 256
                free_best, free_idx = 256, -1                          # (diagnostic: the nearest if nothing had been taken)
                for idx2 in vFeatVec2[f2it][1]:
                    if not vpMapPoints2[idx2]:
                        continue
                    dist = hamming(d1, kf2["desc"][idx2])
                    if dist < free_best:
                        free_best, free_idx = dist, idx2
                    if vbMatched2[idx2]:
                        continue
                    if dist < bestDist1:
                        bestDist2 = bestDist1
                        bestDist1 = dist
                        bestIdx2 = idx2
                    elif dist < bestDist2:
                        bestDist2 = dist
                under = bestDist1 <= th if th_inclusive else bestDist1 < th
                ok = under and bestIdx2 >= 0 and f32(bestDist1) < f32(nn_ratio) * f32(bestDist2)
                info[idx1] = dict(best1=bestDist1, best2=bestDist2, idx=bestIdx2, stolen=free_idx != bestIdx2, ok=bool(ok),
                                  under=bool(under), node=vFeatVec1[f1it][0])
                if ok:
                    vpMatches12[idx1] = bestIdx2
                    dist12[idx1] = bestDist1
                    vbMatched2[bestIdx2] = True
                    if check_orientation:
                        b = rot_bin(kf1["angle"][idx1], kf2["angle"][bestIdx2])
                        if b == HISTO_LENGTH:
                            b = 0
                        assert 0 <= b < HISTO_LENGTH
                        rotHist[b].append(idx1)
                    nmatches += 1
            f1it += 1
            f2it += 1
        elif vFeatVec1[f1it][0] < vFeatVec2[f2it][0]:
            f1it = _lower_bound(vFeatVec1, f1it, vFeatVec2[f2it][0])
        else:
            f2it = _lower_bound(vFeatVec2, f2it, vFeatVec1[f1it][0])
    raw = list(vpMatches12)
    ind = (-1, -1, -1)
    if check_orientation:
        ind = three_maxima([len(h) for h in rotHist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idx1 in rotHist[i]:
                vpMatches12[idx1] = -1
                nmatches -= 1
    r = _result(n1, vpMatches12, raw, dist12, [len(h) for h in rotHist], ind, info)
    assert r["n_matches"] == nmatches
    return r


def literal_frame(kf, fr, th, th_inclusive, nn_ratio, check_orientation):
    """:159-288; vpMapPointMatches[idxF] holds the key frame's index in place of the map point; returned by source (key-frame) slot"""
    vFeatVecKF, vFeatVecF = nodes_of(kf), nodes_of(fr)
    vpMapPointsKF = _eligible(kf)
    elF = _eligible(fr)                                                # all ones in the reference (eligible = None)
    N = len(fr["angle"])
    vpMapPointMatches = [None] * N
    distF = [-1] * N
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    info = {}
    KFit, Fit, KFend, Fend = 0, 0, len(vFeatVecKF), len(vFeatVecF)
    while KFit != KFend and Fit != Fend:
        if vFeatVecKF[KFit][0] == vFeatVecF[Fit][0]:
            vIndicesKF, vIndicesF = vFeatVecKF[KFit][1], vFeatVecF[Fit][1]
            for realIdxKF in vIndicesKF:
                if not vpMapPointsKF[realIdxKF]:
                    continue
                dKF = kf["desc"][realIdxKF]
                bestDist1, bestIdxF, bestDist2 = 256, -1, 256
                free_best, free_idx = 256, -1
                for realIdxF in vIndicesF:
                    if not elF[realIdxF]:
                        continue
                    dist = hamming(dKF, fr["desc"][realIdxF])
                    if dist < free_best:
                        free_best, free_idx = dist, realIdxF
                    if vpMapPointMatches[realIdxF] is not None:
                        continue
                    if dist < bestDist1:
                        bestDist2 = bestDist1
                        bestDist1 = dist
                        bestIdxF = realIdxF
                    elif dist < bestDist2:
                        bestDist2 = dist
                under = bestDist1 <= th if th_inclusive else bestDist1 < th
                ok = under and bestIdxF >= 0 and f32(bestDist1) < f32(nn_ratio) * f32(bestDist2)
                info[realIdxKF] = dict(best1=bestDist1, best2=bestDist2, idx=bestIdxF, stolen=free_idx != bestIdxF, ok=bool(ok),
                                       under=bool(under), node=vFeatVecKF[KFit][0])
                if ok:
                    vpMapPointMatches[bestIdxF] = realIdxKF
                    distF[bestIdxF] = bestDist1
                    if check_orientation:
                        b = rot_bin(kf["angle"][realIdxKF], fr["angle"][bestIdxF])
                        if b == HISTO_LENGTH:
                            b = 0
                        assert 0 <= b < HISTO_LENGTH
                        rotHist[b].append(bestIdxF)
                    nmatches += 1
            KFit += 1
            Fit += 1
        elif vFeatVecKF[KFit][0] < vFeatVecF[Fit][0]:
            KFit = _lower_bound(vFeatVecKF, KFit, vFeatVecF[Fit][0])
        else:
            Fit = _lower_bound(vFeatVecF, Fit, vFeatVecKF[KFit][0])
    before = list(vpMapPointMatches)
    ind = (-1, -1, -1)
    if check_orientation:
        ind = three_maxima([len(h) for h in rotHist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idxF in rotHist[i]:
                vpMapPointMatches[idxF] = None
                nmatches -= 1
    n_src = len(vpMapPointsKF)
    match, raw, dist = [-1] * n_src, [-1] * n_src, [-1] * n_src
    for idxF in range(N):                                              # by source slot
        if before[idxF] is not None:
            raw[before[idxF]] = idxF
            dist[before[idxF]] = distF[idxF]
        if vpMapPointMatches[idxF] is not None:
            match[vpMapPointMatches[idxF]] = idxF
    r = _result(n_src, match, raw, dist, [len(h) for h in rotHist], ind, info)
    assert r["n_matches"] == nmatches
    return r


def literal(shared, cand, shared_is_source=True, th=50, th_inclusive=False, nn_ratio=0.75, check_orientation=True):
    if shared_is_source:
        return literal_kf(shared, cand, th, th_inclusive, nn_ratio, check_orientation)
    return literal_frame(cand, shared, th, th_inclusive, nn_ratio, check_orientation)


def by_sets(shared, cand, shared_is_source=True, th=50, th_inclusive=False, nn_ratio=0.75, check_orientation=True):
    """the same function from sets and sorts: no iterator walk, no running top-2, no index lists"""
    S, T = (shared, cand) if shared_is_source else (cand, shared)
    eS, eT = _eligible(S), _eligible(T)
    nS = len(eS)
    sid, tid = np.asarray(S["node_id"]), np.asarray(T["node_id"])
    so_, to_ = np.asarray(S["node_off"]), np.asarray(T["node_off"])
    common, ks, kt = np.intersect1d(sid, tid, return_indices=True)
    raw, dist = np.full(nS, -1, np.int32), np.full(nS, -1, np.int32)
    free = eT.copy()
    nn = f32(nn_ratio)
    for a, b in zip(ks, kt):
        src = np.asarray(S["feat"][so_[a]:so_[a + 1]], np.int64)
        tgt = np.asarray(T["feat"][to_[b]:to_[b + 1]], np.int64)
        if not len(tgt):
            continue
        D = POP[np.bitwise_xor(np.asarray(S["desc"])[src][:, None, :], np.asarray(T["desc"])[tgt][None, :, :])].sum(-1)
        for row, i in enumerate(src):
            if not eS[i]:
                continue
            live = np.flatnonzero(free[tgt])
            if not len(live):
                continue
            d = D[row, live]
            order = np.argsort(d, kind="stable")
            b1 = int(d[order[0]])
            b2 = int(d[order[1]]) if len(order) > 1 else 256
            if (b1 <= th if th_inclusive else b1 < th) and f32(b1) < nn * f32(b2):
                j = int(tgt[live[order[0]]])
                raw[i], dist[i] = j, b1
                free[j] = False
    match = raw.copy()
    hist, ind = np.zeros(HISTO_LENGTH, np.int32), np.full(3, -1, np.int32)
    if check_orientation:
        m = np.flatnonzero(raw >= 0)
        rot = np.asarray(S["angle"], f32)[m] - np.asarray(T["angle"], f32)[raw[m]]
        rot = np.where(rot < 0, (rot + f32(360.0)).astype(f32), rot).astype(f32)
        bins = np.floor((rot * FACTOR).astype(f32).astype(np.float64) + 0.5).astype(np.int64)
        bins[bins == HISTO_LENGTH] = 0
        hist = np.bincount(bins, minlength=HISTO_LENGTH).astype(np.int32)
        # the three largest counts, earlier bin first among equals (the strict > chain), then the two 0.1f tests
        top = [int(i) for i in np.argsort(-hist, kind="stable")[:3] if hist[i] > 0]
        top += [-1] * (3 - len(top))
        cnt = [int(hist[i]) if i >= 0 else 0 for i in top]
        if f32(cnt[1]) < f32(0.1) * f32(cnt[0]):
            top[1] = top[2] = -1
        elif f32(cnt[2]) < f32(0.1) * f32(cnt[0]):
            top[2] = -1
        ind = np.array(top, np.int32)
        match[m[~np.isin(bins, ind[ind >= 0])]] = -1
    return dict(match=match, match_raw=raw, dist=dist, hist=hist, ind=ind, n_matches=int((match >= 0).sum()))


KEYS = ("match", "match_raw", "dist", "hist", "ind")


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and a["n_matches"] == b["n_matches"]


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def make_frame(desc, angle, nodes, eligible=None):
    """nodes: list of (id, [feature indices]) in ascending id order"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    node_off = np.concatenate([[0], np.cumsum([len(v) for _, v in nodes])]).astype(np.int32)
    feat = np.array([x for _, v in nodes for x in v], np.int32)
    return dict(desc=desc, angle=np.asarray(angle, f32).reshape(-1), eligible=None if eligible is None else np.asarray(eligible, np.uint8),
                node_id=np.array([i for i, _ in nodes], np.int32), node_off=node_off, feat=feat)


def flipped(desc, bits):
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class Builder(object):
    """grows a (source, target) frame pair node by node"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.d = ([], [])
        self.a = ([], [])
        self.e = ([], [])
        self.nodes = ({}, {})
        self.named = {}

    def rand(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def add(self, side, node, desc, angle=0.0, eligible=1, front=False):
        i = len(self.d[side])
        self.d[side].append(np.asarray(desc, np.uint8))
        self.a[side].append(f32(angle))
        self.e[side].append(eligible)
        lst = self.nodes[side].setdefault(node, [])
        lst.insert(0, i) if front else lst.append(i)
        return i

    def frame(self, side, all_eligible=False):
        n = len(self.d[side])
        desc = np.stack(self.d[side]) if n else np.zeros((0, 32), np.uint8)
        return make_frame(desc, self.a[side], sorted(self.nodes[side].items()), None if all_eligible else self.e[side])


def world(seed, n_nodes=24, per_node=9):
    """landmarks: descriptor, vocabulary node, angle; node ids are sparse and ascending"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(3, 900), n_nodes, replace=False))
    L = n_nodes * per_node
    return dict(desc=rng.integers(0, 256, (L, 32)).astype(np.uint8), node=np.repeat(ids, per_node), angle=rng.uniform(0, 360, L).astype(f32))


def observe(w, seed, n, rot=0.0, jitter=2.0, stray=0.0, flips=12, elig=0.85, twins=0, drop_nodes=()):
    """a frame that sees n landmarks of the world: a few bits flipped, angles turned by `rot` (+ jitter; a share `stray` anywhere),
    `twins` extra near-copies of seen landmarks in the same node (what makes sources compete), slots listed per node in index order"""
    rng = np.random.default_rng(seed)
    L = len(w["angle"])
    seen = rng.permutation(L)[:n]
    seen = np.concatenate([seen, rng.choice(seen, twins)]).astype(np.int64) if n and twins else seen
    desc, angle, node = [], [], []
    for l in seen:
        desc.append(flipped(w["desc"][l], rng.choice(256, rng.integers(0, flips + 1), replace=False)))
        a = rng.uniform(0, 360) if rng.uniform() < stray else (float(w["angle"][l]) + rot + rng.normal() * jitter) % 360.0
        angle.append(a)
        node.append(int(w["node"][l]))
    nodes = {}
    for i, k in enumerate(node):
        if k not in drop_nodes:
            nodes.setdefault(k, []).append(i)
    e = (rng.uniform(size=len(seen)) < elig).astype(np.uint8)
    return make_frame(np.array(desc, np.uint8).reshape(-1, 32), angle, sorted(nodes.items()), e)


_CACHE = {}


def cached(fn):
    def get(*a):
        key = (fn.__name__,) + a
        if key not in _CACHE:
            _CACHE[key] = fn(*a)
        return _CACHE[key]
    return get


def _clean_pair(seed, bins_counts, extra_src=0):
    """every source has exactly one exact copy in the target, alone with it in a node of its own: every pair is matched, and
    the angle differences land `count` pairs in bin `b` for every (b, count)"""
    B = Builder(seed)
    node = 10
    for b, count in bins_counts:
        for k in range(count):
            d = B.rand()
            a_t = float(B.rng.uniform(0, 300))
            B.add(0, node, d, (a_t + 30.0 * b + B.rng.uniform(-9, 9)) % 360.0)
            B.add(1, node, d, a_t)
            node += 3
    for _ in range(extra_src):
        B.add(0, node, B.rand(), 0.0)
        node += 3
    return B


@cached
def steal_nodes(with_ratio_fail):
    """node 40: source A (first) takes A' at distance 3; source B's nearest is A' too (12), it then takes B'' at 20.
    with_ratio_fail: a further target at 24 from B makes 20 < 0.75 * 24 false"""
    B = Builder(77 + with_ratio_fail)
    X = B.rand()
    A = X
    Bs = flipped(X, range(100, 109))                                   # 9 from A
    B.named["A"] = B.add(0, 40, A, 50.0)
    B.named["B"] = B.add(0, 40, Bs, 80.0)
    B.named["A'"] = B.add(1, 40, flipped(X, range(0, 3)), 20.0)        # 3 from A, 12 from B
    B.named["B''"] = B.add(1, 40, flipped(Bs, range(200, 220)), 50.0)  # 20 from B, 29 from A
    if with_ratio_fail:
        B.named["B'''"] = B.add(1, 40, flipped(Bs, range(140, 164)), 50.0)   # 24 from B
    for k in range(6):                                                 # bystanders in the node and around it
        B.add(1, 40, B.rand(), 10.0)
        d = B.rand()
        B.add(0, 41 + k, d, 100.0)
        B.add(1, 41 + k, flipped(d, range(0, k)), 70.0)
    return B


@cached
def kf_pool():
    """key-frame mode: the shared key frame 1 and 8 candidates"""
    w = world(1)
    shared = observe(w, 10, 150, twins=20)
    c = [make_frame(np.zeros((0, 32), np.uint8), [], []),                                          # 0: zero key points
         observe(w, 11, 140, rot=40.0, stray=0.25, twins=15),                                      # 1: a rotation cull removes matches
         observe(w, 12, 160, rot=200.0, jitter=25.0, twins=15),                                    # 2: three bins kept
         observe(w, 13, 120, rot=90.0, jitter=1.0, stray=0.04, flips=6),                           # 3: max2 < 0.1 max1
         observe(w, 14, 100, rot=300.0, elig=0.0),                                                 # 4: no eligible target
         observe(w, 15, 300, rot=10.0, twins=40, flips=20),                                        # 5: 300 key points, crowded nodes
         observe(w, 16, 130, rot=355.0, jitter=6.0, drop_nodes=tuple(int(x) for x in np.unique(w["node"])[::3])),   # 6: absent nodes
         observe(w, 17, 64, rot=120.0)]
    return shared, c


@cached
def frame_pool():
    """frame mode: the shared frame (every slot eligible) and 8 candidate key frames, among them one with no eligible slot and one
    with zero key points"""
    w = world(2)
    shared = observe(w, 20, 170, twins=25)
    shared["eligible"] = None
    c = [observe(w, 21, 140, rot=40.0, stray=0.25, twins=15),
         make_frame(np.zeros((0, 32), np.uint8), [], []),                                          # zero key points
         observe(w, 22, 160, rot=200.0, jitter=25.0, twins=15),
         observe(w, 23, 100, rot=300.0, elig=0.0),                                                 # no eligible slot
         observe(w, 24, 120, rot=90.0, jitter=1.0, stray=0.04, flips=6),
         observe(w, 25, 300, rot=10.0, twins=40, flips=20),
         observe(w, 26, 130, rot=355.0, jitter=6.0, drop_nodes=tuple(int(x) for x in np.unique(w["node"])[1::3])),
         observe(w, 27, 63, rot=120.0)]
    return shared, c


EQUAL_BINS = ((2, 6), (5, 6), (7, 6), (9, 6), (11, 2))       # four bins of 6: the strict > keeps 2, 5, 7 and drops 9
SMALL_MAX2 = ((4, 31), (1, 3), (8, 2))                      # 3 < 0.1f * 31: only bin 4 survives


@cached
def lengths_pair():
    """target lists of 0, 1, 63, 64, 65 and 130 entries: three sources per node, the first two compete for one target"""
    B = Builder(5)
    for node, n_t in zip((3, 4, 8, 9, 17, 30), (0, 1, 63, 64, 65, 130)):
        X = B.rand()
        B.add(0, node, X, 10.0)
        B.add(0, node, flipped(X, range(100, 104)), 10.0)
        B.add(0, node, B.rand(), 10.0)
        if n_t == 0:
            B.nodes[1][node] = []
        for k in range(n_t):
            last = k == n_t - 1                                        # the wanted target sits at the END of the list
            B.add(1, node, flipped(X, range(0, 2)) if last else flipped(X, range(30, 60)) if k == 0 else B.rand(), 5.0)
    return B


@cached
def hand_pair():
    """the hand-made cases, one node each (node ids in NODE); distances are set by flipping disjoint bit ranges"""
    B = Builder(9)
    nd = B.named

    def case(name, node, dists, a_src=0.0, a_tgt=0.0):
        X = B.rand()
        nd[name] = B.add(0, node, X, a_src)
        at = 0
        for d in dists:
            nd.setdefault(name + "_t", []).append(B.add(1, node, flipped(X, range(at, at + d)), a_tgt))
            at += d
        return X

    B.add(0, 1, B.rand())                                              # a node only the source holds, before all others
    B.add(1, 2, B.rand())                                              # ... and one only the target holds
    case("d49", 5, [49])
    case("d50", 6, [50])
    case("d51", 7, [51])
    case("r30_40", 8, [30, 40])
    case("equal_minima", 9, [10, 10])
    case("equal_zero", 10, [0, 0])
    B.add(0, 11, B.rand())                                             # one-sided nodes in the middle of the walk
    B.add(1, 12, B.rand())
    B.add(1, 13, B.rand())
    case("single", 14, [49])
    # a tie between list positions p and p + 64 (one lane holds both) and one between different lanes; the earlier wins
    X = B.rand()
    nd["tie_lane"] = B.add(0, 20, X)
    lst = [B.add(1, 20, B.rand()) for _ in range(130)]
    B.d[1][lst[3]] = flipped(X, range(0, 10))
    B.d[1][lst[67]] = flipped(X, range(20, 30))
    nd["tie_lane_first"], nd["tie_lane_second"] = lst[3], lst[67]
    X = B.rand()
    nd["tie_lanes"] = B.add(0, 21, X)
    lst = [B.add(1, 21, B.rand()) for _ in range(12)]
    B.d[1][lst[9]] = flipped(X, range(0, 10))
    B.d[1][lst[5]] = flipped(X, range(20, 30))
    nd["tie_lanes_first"], nd["tie_lanes_second"] = lst[5], lst[9]
    # a feat list that is not ascending: the LISTED order decides who takes the contested target
    X = B.rand()
    late = B.add(0, 22, flipped(X, range(0, 2)))                       # index order: `late` first ...
    early = B.add(0, 22, X, front=True)                                # ... list order: `early` first
    nd["unsorted_early"], nd["unsorted_late"] = early, late
    nd["unsorted_t"] = B.add(1, 22, X)
    B.add(1, 22, B.rand(), front=True)
    # angles
    case("rot_negative", 23, [1], 10.0, 350.0)
    case("rot_zero", 24, [1], 77.0, 77.0)
    case("rot_minus_zero", 25, [1], -0.0, 0.0)
    case("rot_wraps_to_360", 26, [1], 0.0, 1e-6)
    case("rot_half", 27, [1], HALF_ANGLE, 0.0)
    B.add(0, 90, B.rand())                                             # one-sided nodes at the end of the walk
    B.add(1, 95, B.rand())
    return B


def _half_angle():
    """an angle whose float32 product with 1.0f / 30 sits exactly on x.5"""
    for k in range(1, 24, 2):
        a = f32(15.0 * k)
        v = float(f32(a * FACTOR))
        if v - math.floor(v) == 0.5:
            return a
    raise AssertionError("no angle lands on x.5")


HALF_ANGLE = _half_angle()
HAND_PARAMS = (dict(th=50, th_inclusive=False, nn_ratio=0.75), dict(th=50, th_inclusive=True, nn_ratio=0.75),
               dict(th=50, th_inclusive=False, nn_ratio=1.5))


@cached
def big_pair(n_targets):
    """one node of n_targets targets and three sources, the second of which loses its nearest target (the last of the list) to
    the first; a second, ordinary node beside it"""
    B = Builder(100 + n_targets)
    X = B.rand()
    B.named["first"] = B.add(0, 7, X, 30.0)
    B.named["second"] = B.add(0, 7, flipped(X, range(100, 104)), 30.0)
    B.named["third"] = B.add(0, 7, B.rand(), 30.0)
    for k in range(n_targets):
        d = B.rand()
        if k == n_targets - 1:
            d = flipped(X, range(0, 2))                                # 2 from the first, 6 from the second
        elif k == n_targets // 2:
            d = flipped(X, range(96, 120))                             # 24 from the first, 20 from the second (shares 100..103)
        i = B.add(1, 7, d, 0.0)
        if k == n_targets - 1:
            B.named["last"] = i
        elif k == n_targets // 2:
            B.named["middle"] = i
    d = B.rand()
    B.add(0, 9, d, 30.0)
    B.add(1, 9, d, 0.0)
    return B


@cached
def scenes():
    """name -> (shared, [candidates], shared_is_source): every fixture of the CPU and GPU tests, in both modes"""
    out = {}
    s, c = kf_pool()
    out["kf_pool"] = (s, c, True)
    s, c = frame_pool()
    out["frame_pool"] = (s, c, False)
    w = world(1)
    none = observe(w, 30, 120, elig=0.0)
    zero = make_frame(np.zeros((0, 32), np.uint8), [], [])
    two = [observe(w, 31, 90), observe(w, 32, 40)]
    out["kf_source_not_eligible"] = (none, two, True)
    out["kf_source_empty"] = (zero, two, True)
    out["frame_target_empty"] = (zero, two, False)
    for mode, sis in (("kf", True), ("frame", False)):
        pairs = [_clean_pair(3, EQUAL_BINS), _clean_pair(4, SMALL_MAX2, extra_src=5), steal_nodes(0), steal_nodes(1), lengths_pair(), hand_pair()]
        for name, B in zip(("equal_bins", "small_max2", "steal", "steal_ratio", "lengths", "hand"), pairs):
            src, tgt = B.frame(0), B.frame(1, all_eligible=not sis)
            out["%s_%s" % (mode, name)] = ((src, [tgt], True) if sis else (tgt, [src], False))
    return out


def params_of(name):
    """the parameter sets a scene runs under (beside both settings of check_orientation)"""
    if name.endswith("_hand"):
        return HAND_PARAMS
    return (dict(th=50, th_inclusive=not name.startswith("kf"), nn_ratio=0.75),)


@cached
def expected(name, p_index, check_orientation):
    shared, cands, sis = scenes()[name]
    p = params_of(name)[p_index]
    return [literal(shared, c, shared_is_source=sis, check_orientation=bool(check_orientation), **p) for c in cands]
