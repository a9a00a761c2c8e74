"""Two restatements of the reference's place recognition, and the scenes the tests run them on.

`Literal` is written from the reference line by line: KeyFrameDatabase::add / erase / clear / DetectLoopCandidates /
DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-309), the minimum-score loop of LoopClosing::DetectLoop
(src/LoopClosing.cc:131-148) and DBoW2's L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): an inverted file of
Python lists, mutable per-key-frame state.  Doubles are Python floats; floats go through np.float32 after every operation.
`Flat` is the formulation the device uses: no inverted file, intersection sizes and the (first common word, list sequence) order.

The three deviations of include/qsp_hip.h hold for both: scores start at 0.0f, every call is a new query (the stamp is a counter,
not the querying frame's id), and the frame-id-0 quirk is not reproduced.

A HISTORY is a list of operations -- ("put", id, words, values, listed), ("list", id), ("erase", id), ("clear",),
("query", mode, words, values, dict(excluded=, min_score=, ref_ids=), neighbours) with neighbours a dict id -> ids of
GetBestCovisibilityKeyFrames(10) -- and run_history(db, ops) returns the result of every query: the taps of qsp_place_db_query and
qsp_place_db_accumulate under the names of KEYS."""
import bisect

import numpy as np

f32 = np.float32
LOOP, RELOC = 0, 1
KEYS = ("n_sharing", "max_common", "min_common", "min_score_used", "match_id", "match_score", "sharing_id", "sharing_common",
        "sharing_first", "cand_id", "acc_score", "best_id")


def l1_score(v1, v2):
    """ScoringObject.cpp:23-68; v1, v2: (sorted word list, value list) -- the std::map walked with its two lower_bound jumps"""
    w1, x1 = v1
    w2, x2 = v2
    i = j = 0
    score = 0.0
    while i < len(w1) and j < len(w2):
        vi, wi = x1[i], x2[j]
        if w1[i] == w2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j])
        else:
            j = bisect.bisect_left(w2, w1[i])
    score = -score / 2.0
    return score


class _KF(object):
    def __init__(self, kf_id, words, values):
        self.id = kf_id
        self.bow = ([int(w) for w in words], [float(v) for v in values])
        self.loop_query = self.reloc_query = 0             # 0: never (the query counter starts at 1)
        self.loop_words = self.reloc_words = 0
        self.loop_score = self.reloc_score = f32(0)
        self.listed = False
        self.seq = -1


def _result(**kw):
    r = dict(n_sharing=0, max_common=0, min_common=0, min_score_used=f32(0), match_id=[], match_score=[], sharing_id=[],
             sharing_common=[], sharing_first=[], cand_id=[], acc_score=[], best_id=[])
    r.update(kw)
    return dict(n_sharing=int(r["n_sharing"]), max_common=int(r["max_common"]), min_common=int(r["min_common"]),
                min_score_used=f32(r["min_score_used"]), match_id=np.array(r["match_id"], np.int64),
                match_score=np.array(r["match_score"], f32), sharing_id=np.array(r["sharing_id"], np.int64),
                sharing_common=np.array(r["sharing_common"], np.int32), sharing_first=np.array(r["sharing_first"], np.int32),
                cand_id=np.array(r["cand_id"], np.int64), acc_score=np.array(r["acc_score"], f32), best_id=np.array(r["best_id"], np.int64))


class _Base(object):
    def __init__(self):
        self.clear()

    def clear(self):
        self.known = {}
        self.inverted = {}
        self.n_query = 0
        self.n_seq = 0

    def put(self, kf_id, words, values, listed=True):
        assert kf_id not in self.known
        self.known[kf_id] = _KF(kf_id, words, values)
        if listed:
            self.list(kf_id)

    def erase(self, kf_id):
        kf = self.known.pop(kf_id, None)
        if kf is not None and kf.listed:
            self._unlist(kf)

    def min_score(self, query, ref_ids):
        """LoopClosing.cc:136-148 (the caller has left the bad key frames out)"""
        m = f32(1)
        for r in ref_ids:
            score = f32(l1_score(query, self.known[r].bow))
            if score < m:
                m = score
        return m

    def detect(self, mode, words, values, neighbours, excluded=(), min_score=0.0, ref_ids=None):
        query = ([int(w) for w in words], [float(v) for v in values])
        if mode == LOOP:
            ms = self.min_score(query, ref_ids) if ref_ids is not None and len(ref_ids) else f32(min_score)
            return self.detect_loop(query, set(int(e) for e in excluded), ms, neighbours)
        return self.detect_reloc(query, neighbours)

    def _accumulate(self, mode, q, lScoreAndMatch, minCommonWords, start, neighbours):
        """:144-196 / :258-308"""
        lAcc = []
        bestAccScore = f32(start)
        for si, kf in lScoreAndMatch:
            bestScore = si
            accScore = si
            best = kf
            for n_id in neighbours[kf.id]:
                kf2 = self.known.get(n_id)
                if kf2 is None:                            # unknown or erased: not of this query
                    continue
                if mode == LOOP:
                    if not (kf2.loop_query == q and kf2.loop_words > minCommonWords):
                        continue
                    s2 = kf2.loop_score
                else:
                    if kf2.reloc_query != q:
                        continue
                    s2 = kf2.reloc_score
                accScore = f32(accScore + s2)
                if s2 > bestScore:
                    best = kf2
                    bestScore = s2
            lAcc.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        already, cands = set(), []
        for a, kf in lAcc:
            if a > minScoreToRetain and kf.id not in already:
                cands.append(kf.id)
                already.add(kf.id)
        return dict(cand_id=cands, acc_score=[a for a, _ in lAcc], best_id=[k.id for _, k in lAcc])


class Literal(_Base):
    def list(self, kf_id):
        kf = self.known[kf_id]
        assert not kf.listed
        kf.listed = True
        for w in kf.bow[0]:                                # :44-45
            self.inverted.setdefault(w, []).append(kf)

    def _unlist(self, kf):
        for w in kf.bow[0]:                                # :53-66
            lst = self.inverted.get(w, [])
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break

    def detect_loop(self, query, connected, minScore, neighbours):
        self.n_query += 1
        q = self.n_query
        sharing, first = [], {}
        for w in query[0]:                                 # :86-104
            for kf in self.inverted.get(w, []):
                if kf.loop_query != q:
                    kf.loop_words = 0
                    if kf.id not in connected:
                        kf.loop_query = q
                        sharing.append(kf)
                        first[kf.id] = w
                kf.loop_words += 1
        if not sharing:
            return _result(min_score_used=minScore)
        maxCommonWords = 0
        for kf in sharing:
            if kf.loop_words > maxCommonWords:
                maxCommonWords = kf.loop_words
        minCommonWords = int(f32(f32(maxCommonWords) * f32(0.8)))
        lScoreAndMatch = []
        for kf in sharing:                                 # :125-139
            if kf.loop_words > minCommonWords:
                si = f32(l1_score(query, kf.bow))
                kf.loop_score = si
                if si >= minScore:
                    lScoreAndMatch.append((si, kf))
        taps = dict(n_sharing=len(sharing), max_common=maxCommonWords, min_common=minCommonWords, min_score_used=minScore,
                    sharing_id=[k.id for k in sharing], sharing_common=[k.loop_words for k in sharing],
                    sharing_first=[first[k.id] for k in sharing], match_id=[k.id for _, k in lScoreAndMatch],
                    match_score=[s for s, _ in lScoreAndMatch])
        if lScoreAndMatch:
            taps.update(self._accumulate(LOOP, q, lScoreAndMatch, minCommonWords, minScore, neighbours))
        return _result(**taps)

    def detect_reloc(self, query, neighbours):
        self.n_query += 1
        q = self.n_query
        sharing, first = [], {}
        for w in query[0]:                                 # :207-222
            for kf in self.inverted.get(w, []):
                if kf.reloc_query != q:
                    kf.reloc_words = 0
                    kf.reloc_query = q
                    sharing.append(kf)
                    first[kf.id] = w
                kf.reloc_words += 1
        if not sharing:
            return _result()
        maxCommonWords = 0
        for kf in sharing:
            if kf.reloc_words > maxCommonWords:
                maxCommonWords = kf.reloc_words
        minCommonWords = int(f32(f32(maxCommonWords) * f32(0.8)))
        lScoreAndMatch = []
        for kf in sharing:                                 # :242-253
            if kf.reloc_words > minCommonWords:
                si = f32(l1_score(query, kf.bow))
                kf.reloc_score = si
                lScoreAndMatch.append((si, kf))
        taps = dict(n_sharing=len(sharing), max_common=maxCommonWords, min_common=minCommonWords,
                    sharing_id=[k.id for k in sharing], sharing_common=[k.reloc_words for k in sharing],
                    sharing_first=[first[k.id] for k in sharing], match_id=[k.id for _, k in lScoreAndMatch],
                    match_score=[s for s, _ in lScoreAndMatch])
        if lScoreAndMatch:
            taps.update(self._accumulate(RELOC, q, lScoreAndMatch, minCommonWords, 0, neighbours))
        return _result(**taps)


class Flat(_Base):
    """What the device does: per listed key frame the intersection with the query, the sharing ones sorted by (first common word,
    list sequence number), the score as a serial sum over the common words ascending."""

    def list(self, kf_id):
        kf = self.known[kf_id]
        assert not kf.listed
        kf.listed = True
        kf.seq = self.n_seq
        self.n_seq += 1

    def _unlist(self, kf):
        kf.listed = False

    @staticmethod
    def _score(query, kf, common):
        qv = dict(zip(*query))
        kv = dict(zip(*kf.bow))
        s = 0.0
        for w in common:
            s += abs(qv[w] - kv[w]) - abs(qv[w]) - abs(kv[w])
        return f32(-s / 2.0)

    def _query(self, mode, query, connected, minScore):
        self.n_query += 1
        q = self.n_query
        qs = set(query[0])
        sharing = []
        for kf in self.known.values():
            if not kf.listed or (mode == LOOP and kf.id in connected):
                continue
            common = sorted(qs.intersection(kf.bow[0]))
            if not common:
                continue
            if mode == LOOP:
                kf.loop_query, kf.loop_words = q, len(common)
            else:
                kf.reloc_query, kf.reloc_words = q, len(common)
            sharing.append(((common[0], kf.seq), kf, common))
        sharing.sort(key=lambda t: t[0])
        maxc = max([len(c) for _, _, c in sharing] + [0])
        minc = int(f32(f32(maxc) * f32(0.8)))
        ls = []
        for _, kf, common in sharing:
            if len(common) > minc:
                si = self._score(query, kf, common)
                if mode == LOOP:
                    kf.loop_score = si
                    if si >= minScore:
                        ls.append((si, kf))
                else:
                    kf.reloc_score = si
                    ls.append((si, kf))
        taps = dict(n_sharing=len(sharing), max_common=maxc, min_common=minc, min_score_used=minScore if mode == LOOP else 0,
                    sharing_id=[k.id for _, k, _ in sharing], sharing_common=[len(c) for _, _, c in sharing],
                    sharing_first=[c[0] for _, _, c in sharing], match_id=[k.id for _, k in ls], match_score=[s for s, _ in ls])
        return q, ls, minc, taps

    def detect_loop(self, query, connected, minScore, neighbours):
        q, ls, minc, taps = self._query(LOOP, query, connected, minScore)
        if ls:
            taps.update(self._accumulate(LOOP, q, ls, minc, minScore, neighbours))
        return _result(**taps)

    def detect_reloc(self, query, neighbours):
        q, ls, minc, taps = self._query(RELOC, query, (), f32(0))
        if ls:
            taps.update(self._accumulate(RELOC, q, ls, minc, 0, neighbours))
        return _result(**taps)


def run_history(db, ops):
    out = []
    for op in ops:
        if op[0] == "put":
            db.put(op[1], op[2], op[3], listed=op[4])
        elif op[0] == "list":
            db.list(op[1])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        else:
            out.append(db.detect(op[1], op[2], op[3], op[5], **op[4]))
    return out


def differing(got, want):
    """the count of entries that differ over every tap (a length mismatch counts every entry of the longer); floats as bits"""
    n = 0
    for k in KEYS:
        g, w = np.atleast_1d(np.asarray(got[k])), np.atleast_1d(np.asarray(want[k]))
        if w.dtype == np.float32:
            g, w = g.astype(np.float32).view(np.uint32), w.view(np.uint32)
        if g.shape != w.shape:
            n += max(g.size, w.size, 1)
        else:
            n += int((g != w).sum())
    return n


# ---- scenes --------------------------------------------------------------------------------------------------------------------
class AnyNeighbours(dict):
    """a neighbour table that answers every id: the given lists, else none"""
    def __missing__(self, key):
        return []


def bow(rng, n, vocab):
    """n words of range(vocab), ascending, with tf-idf-like positive weights that sum to 1"""
    w = np.sort(rng.choice(vocab, n, replace=False)).astype(np.int32)
    v = rng.gamma(2.0, 1.0, n) * rng.uniform(0.2, 9.0, n)
    return w, (v / v.sum() if n else v).astype(np.float64)


def _q(mode, wv, nb=None, **kw):
    return ("query", mode, wv[0], wv[1], kw, AnyNeighbours(nb or {}))


def _put(i, wv, listed=True):
    return ("put", i, wv[0], wv[1], listed)


def _with(table, extra):
    t = dict(table)
    t.update(extra)
    return t


def _dy(words, values):
    return np.array(words, np.int32), np.array(values, np.float64)


def _score_of(q, k):
    return f32(l1_score((list(map(int, q[0])), list(map(float, q[1]))), (list(map(int, k[0])), list(map(float, k[1])))))


def scenes():
    """name -> history.  Each is the smallest that can go wrong in its own way."""
    S = {}
    rng = np.random.default_rng(11)
    pool = [bow(rng, int(n), 40) for n in rng.integers(3, 20, 8)]
    base = [_put(10 + i, p) for i, p in enumerate(pool)]
    nb_all = {10 + i: [10 + (i + d) % 8 for d in (1, 3, 5)] for i in range(8)}
    some = bow(rng, 12, 40)
    empty = _dy([], [])
    S["empty_query"] = base + [_q(LOOP, empty, nb_all, min_score=0.0), _q(RELOC, empty, nb_all), _q(LOOP, empty, nb_all, ref_ids=[10, 11])]
    S["empty_database"] = [_q(LOOP, some, min_score=0.01), _q(RELOC, some)] + base + [("clear",), _q(LOOP, some, min_score=0.0), _q(RELOC, some)]
    S["key_frame_of_0_words"] = base[:3] + [_put(30, empty), _put(31, empty, listed=False)] + base[3:] + [
        _q(LOOP, some, _with(nb_all, {10: [30, 31, 11]}), min_score=0.0), _q(RELOC, some, nb_all), _q(LOOP, some, nb_all, ref_ids=[30, 12]),
        _q(LOOP, some, nb_all, ref_ids=[31])]
    # the wave edge and many chunks: every size against every size
    sizes = (63, 64, 65, 4097)
    big = {n: bow(rng, n, int(1.5 * n) + 40) for n in sizes}
    ops = [_put(n, big[n]) for n in sizes] + [_put(7, bow(rng, 64, 136)), _put(8, _dy([5000], [1.0]))]
    nbs = {n: [m for m in sizes if m != n] + [7] for n in sizes}
    for n in sizes:
        qv = bow(rng, n, int(1.5 * n) + 40)
        ops += [_q(LOOP, qv, nbs, min_score=0.0), _q(RELOC, qv, nbs), _q(LOOP, qv, nbs, ref_ids=[4097, 63], excluded=[64])]
    S["wave_edges_63_64_65_4097"] = ops
    S["all_excluded"] = base + [_q(LOOP, some, nb_all, excluded=[10 + i for i in range(8)] + [999], min_score=0.0),
                                _q(LOOP, some, nb_all, excluded=[10 + i for i in range(7)], min_score=0.0)]
    # 0.8f truncation: max_common 5, 10, 15 give 4, 8, 12, and a key frame AT that count is not scored
    for m, t in ((5, 4), (10, 8), (15, 12)):
        qv = _dy(range(m), [1.0 / m] * m)
        kf = lambda k, shift=0.0: _dy(list(range(k)) + [100 + k], [(1.0 - 0.2 - shift) / k] * k + [0.2 + shift])
        S["truncation_max_common_%d" % m] = [_put(1, kf(t, 0.01)), _put(2, kf(m)), _put(3, kf(t + 1, 0.02)), _put(4, kf(t - 1, 0.03)),
                                             _q(LOOP, qv, {2: [1, 3, 4], 3: [2, 1]}, min_score=0.0), _q(RELOC, qv, {2: [1, 3, 4], 3: [2, 1]})]
    # exact ties on dyadic numbers: the score of (word 0, value v) against the query (word 0, 1.0) is exactly v
    one = _dy([0], [1.0])
    kv = lambda v: _dy([0], [v])
    S["score_equal_to_min_score_is_kept"] = [_put(1, kv(0.5)), _put(2, kv(0.25)), _put(3, kv(0.2499999)), _put(4, kv(0.75)),
                                             _q(LOOP, one, {}, min_score=0.25), _q(LOOP, one, {}, ref_ids=[4, 2, 1])]
    S["acc_equal_to_retain_is_dropped"] = [_put(1, kv(0.5)), _put(2, kv(0.375)), _put(3, kv(0.3750001)), _q(RELOC, one, {}),
                                           _q(LOOP, one, {}, min_score=0.125)]
    S["two_entries_one_best"] = [_put(1, kv(0.25)), _put(2, kv(0.3125)), _put(3, kv(0.5)), _q(RELOC, one, {1: [3], 2: [3, 1]}),
                                 _q(LOOP, one, {1: [3], 2: [3, 1]}, min_score=0.0)]
    S["list_order_is_not_id_order"] = [_put(9, pool[0]), _put(3, pool[0]), _put(7, pool[0], listed=False), _put(5, pool[1]), ("list", 7),
                                       _q(LOOP, pool[0], {9: [3], 3: [7]}, min_score=0.0), _q(RELOC, pool[0], {9: [3], 3: [7]})]
    S["erase_in_the_middle_then_put"] = base[:5] + [("erase", 12), ("erase", 555)] + base[5:] + [
        _q(LOOP, some, nb_all, min_score=0.0), _put(12, pool[2]), _q(RELOC, some, nb_all), ("erase", 10), ("erase", 17),
        _q(LOOP, some, nb_all, min_score=0.0)]
    S["unlisted_ref_then_listed"] = base[:4] + [_put(50, some, listed=False),
                                                _q(LOOP, some, _with(nb_all, {10: [50, 11]}), ref_ids=[50, 11], excluded=[50]),
                                                _q(RELOC, some, nb_all), ("list", 50), _q(LOOP, some, _with(nb_all, {10: [50, 11]}), ref_ids=[11, 50]),
                                                _q(RELOC, some, _with(nb_all, {10: [50]}))]
    far = _dy([39000, 39001], [0.5, 0.5])
    S["neighbours_excluded_unknown_erased_not_sharing"] = base + [_put(60, far), _put(61, some), ("erase", 61),
                                                                  _q(LOOP, some, {k: [11, 999, 61, 60, 12, 13] for k in nb_all}, excluded=[11],
                                                                     min_score=0.0),
                                                                  _q(RELOC, some, {k: [11, 999, 61, 60, 12, 13] for k in nb_all})]
    S["ref_without_common_word"] = base + [_put(60, far), _q(LOOP, some, nb_all, ref_ids=[60]), _q(LOOP, some, nb_all, ref_ids=[10, 60, 11])]
    S["stale_reloc_score"] = stale_reloc_scene()
    return S


def stale_reloc_scene():
    """Query 1 scores key frame B (id 2).  Query 2 shares one word with B and many with A (id 1): B is stamped but not scored, and
    as A's neighbour it adds the score that query 1 left."""
    A = _dy(range(10, 30), [0.05] * 20)
    B = _dy([5, 6, 7, 8, 10], [0.2] * 5)
    q1 = _dy([5, 6, 7, 8], [0.25] * 4)
    q2 = _dy(range(10, 30), [0.05] * 20)
    return [_put(1, A), _put(2, B), _q(RELOC, q1, {}), _q(RELOC, q2, {1: [2]}), _q(LOOP, q1, {}, min_score=0.0),
            _q(LOOP, q2, {1: [2]}, min_score=0.0)]


def random_history(seed):
    """0-40 key frames of 0-30 words from a vocabulary of 50 (dense intersections and ties), puts listed or not, lists, erases, a
    clear now and then, and queries of both modes with every kind of minimum score, exclusion and neighbour"""
    rng = np.random.default_rng(1000 + seed)
    n_kf = int(rng.integers(0, 41))
    ops, known, listed, ever = [], set(), set(), []
    next_id = 0

    def a_bow():
        return bow(rng, int(rng.integers(0, 31)), 50)

    def a_query():
        ids = ever + [9999]
        nb = AnyNeighbours({i: [int(x) for x in rng.choice(ids, int(rng.integers(0, 11)))] for i in ever})
        wv = a_bow()
        if rng.uniform() < 0.5:
            return _q(RELOC, wv, nb)
        kw = dict(excluded=[int(x) for x in rng.choice(ids, int(rng.integers(0, 6)))])
        kind = rng.integers(0, 3)
        if kind == 0 and known:
            kw["ref_ids"] = [int(x) for x in rng.choice(sorted(known), int(rng.integers(1, 5)))]
        elif kind == 1:
            kw["min_score"] = float(f32(rng.uniform(0, 0.3)))
        else:
            kw["min_score"] = 0.0
        return ("query", LOOP, wv[0], wv[1], kw, nb)

    for _ in range(n_kf):
        r = rng.uniform()
        ops.append(_put(next_id, a_bow(), listed=bool(r < 0.8)))
        known.add(next_id)
        ever.append(next_id)
        if r < 0.8:
            listed.add(next_id)
        next_id += 1
        r = rng.uniform()
        if r < 0.15 and known - listed:
            k = int(rng.choice(sorted(known - listed)))
            ops.append(("list", k))
            listed.add(k)
        elif r < 0.3 and known:
            k = int(rng.choice(sorted(known)))
            ops.append(("erase", k))
            known.discard(k)
            listed.discard(k)
        elif r < 0.32:
            ops.append(("clear",))
            known.clear()
            listed.clear()
        if rng.uniform() < 0.3:
            ops.append(a_query())
    ops += [a_query() for _ in range(4)]
    return ops


LARGE_SIZES = (1023, 1024, 1025, 2500)
_LARGE = {}


def large_scene(n):
    """n listed key frames of 4 words out of 12 (dense first-word ties), list order different from id order, every one sharing with
    both queries: the single-workgroup kernels of the device take entries 1024 at a time, and these stand on both sides of that.
    Query 1 (words 0..8) scores about a quarter of them; query 2 (all 12 words) scores every one, so lScoreAndMatch and the
    covisibility pass hold n entries (RELOC) or n less the excluded (LOOP)."""
    if n in _LARGE:
        return _LARGE[n]
    rng = np.random.default_rng(7000 + n)
    ids = [int(x) for x in rng.permutation(n) + 100]
    ops = [_put(i, bow(rng, 4, 12)) for i in ids]
    nb = AnyNeighbours({i: [int(x) for x in rng.choice(ids, 3)] for i in ids})
    v9, v12 = rng.uniform(0.5, 1.5, 9), rng.uniform(0.5, 1.5, 12)
    q9, q12 = _dy(range(9), v9 / v9.sum()), _dy(range(12), v12 / v12.sum())
    ops += [_q(RELOC, q9, nb), _q(LOOP, q9, nb, excluded=[ids[0], ids[n // 2]], ref_ids=[ids[1], ids[2]]),
            _q(RELOC, q12, nb), _q(LOOP, q12, nb, excluded=[ids[5]], min_score=0.0)]
    _LARGE[n] = ops
    return ops
