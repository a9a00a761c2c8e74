"""A numpy restatement of Sim3Solver (reference src/Sim3Solver.cc: constructor :37-112, ComputeSim3 :226-337, CheckInliers :340-364,
Project :382-403), the yardstick of qsp_sim3_ransac_batch, plus the fixtures its tests share.  Written here from the formulas; one
evaluation covers all hypotheses of a candidate at once (arrays lead with the hypothesis index).

Two flavours:
  "f32"  the reference's float32 arithmetic in its operation order: cv::Mat float products of small matrices are row sums in
         double rounded to float32, scaled matrices are one double multiply rounded to float32, cv::eigen on the
         float 4x4 is a Jacobi iteration in float32, norm / atan2 / Rodrigues work in double and store float32;
  "f64"  everything in float64 from the float32 inputs, in the operation order of csrc/sim3_ransac.hpp.
The eigen solver is the same cyclic Jacobi in both (8 sweeps, the first of equal eigenvalues wins): which vector of a degenerate
eigenspace a solver returns is its own accident -- the reference's included -- so the degenerate fixtures below are those where
the outcome does not depend on it (see degenerate_candidate)."""
import functools
import os

import numpy as np

f32, f64 = np.float32, np.float64
SWEEPS = 8
MIN_INLIERS = 20


def _rowdot(A, B, F):
    """sum_k A[..., k] * B[..., k] the way OpenCV's small-matrix product leaves it: summed in double, rounded to F"""
    a, b = A.astype(f64), B.astype(f64)
    s = a[..., 0] * b[..., 0]
    for k in range(1, A.shape[-1]):
        s = s + a[..., k] * b[..., k]
    return s.astype(F)


def _jacobi(A, F):
    """eigenvector of the largest eigenvalue of the symmetric 4x4 matrices A (H,4,4), cyclic Jacobi in F"""
    A = A.astype(F).copy()
    H = len(A)
    V = np.zeros((H, 4, 4), F)
    V[:, range(4), range(4)] = 1
    one = F(1)
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            apq = A[:, p, q].copy()
            on = apq != 0                                          # (NaN != 0: a NaN matrix rotates into NaNs)
            theta = (A[:, q, q] - A[:, p, p]) / (F(2) * apq)
            t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            c = one / np.sqrt(t * t + one)
            s = t * c
            c, s, t = np.where(on, c, one), np.where(on, s, F(0)), np.where(on, t, F(0))
            for k in range(4):
                if k in (p, q):
                    continue
                akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                A[:, k, p] = A[:, p, k] = np.where(on, c * akp - s * akq, akp)
                A[:, k, q] = A[:, q, k] = np.where(on, s * akp + c * akq, akq)
            A[:, p, p] = np.where(on, A[:, p, p] - t * apq, A[:, p, p])
            A[:, q, q] = np.where(on, A[:, q, q] + t * apq, A[:, q, q])
            A[:, p, q] = A[:, q, p] = np.where(on, F(0), apq)
            for k in range(4):
                vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                V[:, k, p] = np.where(on, c * vkp - s * vkq, vkp)
                V[:, k, q] = np.where(on, s * vkp + c * vkq, vkq)
    best, e = A[:, 0, 0].copy(), V[:, :, 0].copy()
    for j in range(1, 4):
        up = A[:, j, j] > best
        best = np.where(up, A[:, j, j], best)
        e = np.where(up[:, None], V[:, :, j], e)
    return e


def _rodrigues(rv):
    """cv::Rodrigues, vector -> matrix, in double"""
    theta = np.sqrt((rv[:, 0] * rv[:, 0] + rv[:, 1] * rv[:, 1]) + rv[:, 2] * rv[:, 2])
    c, s, it = np.cos(theta), np.sin(theta), 1.0 / theta
    r = rv * it[:, None]
    R = np.zeros((len(rv), 3, 3))
    rx = np.zeros((len(rv), 3, 3))
    rx[:, 0, 1], rx[:, 0, 2], rx[:, 1, 0], rx[:, 1, 2], rx[:, 2, 0], rx[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    for i in range(3):
        for j in range(3):
            R[:, i, j] = ((c if i == j else 0.0) + (1.0 - c) * (r[:, i] * r[:, j])) + s * rx[:, i, j]
    small = theta < np.finfo(f64).eps
    R[small] = np.eye(3)
    return R


def horn(X1, X2, tri, fix_scale, flavour):
    """ComputeSim3 for the triples tri (H,3) over the matches X1, X2 (n,3) float32.  Returns R (H,3,3), t (H,3), s (H,), T12,
    T21 (H,3,4) in the flavour's type."""
    F = f32 if flavour == "f32" else f64
    P1, P2 = X1[tri].astype(F), X2[tri].astype(F)                  # (H, point, coordinate)
    if F is f32:
        O1 = (((P1[:, 0] + P1[:, 1]) + P1[:, 2]).astype(f64) * (1.0 / 3)).astype(F)      # cv::reduce in float, C / P.cols a scaling
        O2 = (((P2[:, 0] + P2[:, 1]) + P2[:, 2]).astype(f64) * (1.0 / 3)).astype(F)
    else:
        O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / 3.0
        O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / 3.0
    P1, P2 = P1 - O1[:, None], P2 - O2[:, None]
    H = len(tri)
    M = np.zeros((H, 3, 3), F)
    for i in range(3):
        for j in range(3):
            M[:, i, j] = _rowdot(P2[:, :, i], P1[:, :, j], F)
    m = M.astype(f64) if F is f32 else M                            # N11.. are doubles of the float entries
    N = np.zeros((H, 4, 4), f64)
    N[:, 0, 0] = (m[:, 0, 0] + m[:, 1, 1]) + m[:, 2, 2]
    N[:, 0, 1] = m[:, 1, 2] - m[:, 2, 1]
    N[:, 0, 2] = m[:, 2, 0] - m[:, 0, 2]
    N[:, 0, 3] = m[:, 0, 1] - m[:, 1, 0]
    N[:, 1, 1] = (m[:, 0, 0] - m[:, 1, 1]) - m[:, 2, 2]
    N[:, 1, 2] = m[:, 0, 1] + m[:, 1, 0]
    N[:, 1, 3] = m[:, 2, 0] + m[:, 0, 2]
    N[:, 2, 2] = (-m[:, 0, 0] + m[:, 1, 1]) - m[:, 2, 2]
    N[:, 2, 3] = m[:, 1, 2] + m[:, 2, 1]
    N[:, 3, 3] = (-m[:, 0, 0] - m[:, 1, 1]) + m[:, 2, 2]
    for i in range(4):
        for j in range(i):
            N[:, i, j] = N[:, j, i]
    e = _jacobi(N, F).astype(f64)
    nv = np.sqrt((e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]) + e[:, 3] * e[:, 3])
    ang = np.arctan2(nv, e[:, 0])
    if F is f32:
        rv = (e[:, 1:] * ((2.0 * ang) / nv)[:, None]).astype(F).astype(f64)              # vec = 2*ang*vec/norm(vec): one scaling
    else:
        rv = ((2.0 * ang)[:, None] * e[:, 1:]) / nv[:, None]
    R = _rodrigues(rv).astype(F)
    if fix_scale:
        s = np.ones(H, F)
    else:
        nom, den = np.zeros(H), np.zeros(H)
        for i in range(3):
            for k in range(3):
                p3 = _rowdot(R[:, i, :], P2[:, k, :], F)
                nom = nom + P1[:, k, i].astype(f64) * p3.astype(f64)
                den = den + (p3 * p3).astype(f64)                  # cv::pow(P3, 2, aux_P3) squares in the matrix type
        s = (nom / den).astype(F)
    s64 = s.astype(f64)
    if F is f32:
        sR = (R.astype(f64) * s64[:, None, None]).astype(F)
        t = O1 - (np.stack([_rowdot(R[:, i, :], O2, f64) for i in range(3)], -1) * s64[:, None]).astype(F)
        sRi = (np.swapaxes(R, 1, 2).astype(f64) * (1.0 / s64)[:, None, None]).astype(F)
        ti = (-np.stack([_rowdot(sRi[:, i, :], t, f64) for i in range(3)], -1)).astype(F)
    else:
        sR = s[:, None, None] * R
        t = O1 - np.stack([(sR[:, i, 0] * O2[:, 0] + sR[:, i, 1] * O2[:, 1]) + sR[:, i, 2] * O2[:, 2] for i in range(3)], -1)
        sRi = (1.0 / s)[:, None, None] * np.swapaxes(R, 1, 2)
        ti = -np.stack([(sRi[:, i, 0] * t[:, 0] + sRi[:, i, 1] * t[:, 1]) + sRi[:, i, 2] * t[:, 2] for i in range(3)], -1)
    return R, t, s, np.concatenate([sR, t[:, :, None]], -1), np.concatenate([sRi, ti[:, :, None]], -1)


def _to_image(X, K, F):
    invz = F(1) / X[..., 2]
    return np.stack([K[0] * (X[..., 0] * invz) + K[2], K[1] * (X[..., 1] * invz) + K[3]], -1)


def _project(T, X, K, F):
    """Project(): T (H,3,4), X (n,3) -> (H,n,2)"""
    if F is f32:
        c = np.stack([_rowdot(T[:, None, r, :3], X[None, :, :], F) + T[:, None, r, 3] for r in range(3)], -1)
    else:
        c = np.stack([((T[:, None, r, 0] * X[None, :, 0] + T[:, None, r, 1] * X[None, :, 1]) + T[:, None, r, 2] * X[None, :, 2])
                      + T[:, None, r, 3] for r in range(3)], -1)
    return _to_image(c, K, F)


def _sq(d, F):
    return (d[..., 0].astype(f64) * d[..., 0].astype(f64) + d[..., 1].astype(f64) * d[..., 1].astype(f64)).astype(F)


def evaluate(c, fix_scale, flavour):
    """every hypothesis of candidate c (its triples, all of them): count (H,), flags (H,n), R, t, s, T12, and the errors err1, err2
    (H,n) next to max1, max2 (n,)"""
    F = f32 if flavour == "f32" else f64
    X1, X2 = np.asarray(c["X1c"], f32).reshape(-1, 3), np.asarray(c["X2c"], f32).reshape(-1, 3)
    tri = np.asarray(c["triples"], np.int64).reshape(-1, 3)
    n, H = len(X1), len(tri)
    K1, K2 = np.asarray(c["K1"], f32).astype(F), np.asarray(c["K2"], f32).astype(F)
    max1 = (9.210 * np.asarray(c["sigma2_1"], f32).astype(f64)).astype(F)
    max2 = (9.210 * np.asarray(c["sigma2_2"], f32).astype(f64)).astype(F)
    if H == 0 or n == 0:
        z = np.zeros((H, n))
        return dict(count=np.zeros(H, np.int64), flags=z.astype(bool), R=np.zeros((H, 3, 3), F), t=np.zeros((H, 3), F), s=np.zeros(H, F),
                    T12=np.zeros((H, 3, 4), F), err1=z, err2=z, max1=max1, max2=max2)
    with np.errstate(all="ignore"):
        R, t, s, T12, T21 = horn(X1, X2, tri, fix_scale, flavour)
        x1, x2 = X1.astype(F), X2.astype(F)
        p1, p2 = _to_image(x1, K1, F), _to_image(x2, K2, F)
        err1 = _sq(p1[None] - _project(T12, x2, K1, F), F)
        err2 = _sq(_project(T21, x1, K2, F) - p2[None], F)
        flags = (err1 < max1[None]) & (err2 < max2[None])
    return dict(count=flags.sum(1), flags=flags, R=R, t=t, s=s, T12=T12, err1=err1, err2=err2, max1=max1, max2=max2)


def edge(r):
    """the knife-edge distance of every (hypothesis, match) pair of an "f64" evaluation: min(|err1 - max1| / max1, |err2 - max2| /
    max2); a pair whose errors are NaN is an outlier whatever the rounding: inf"""
    with np.errstate(all="ignore"):
        d = np.minimum(np.abs(r["err1"] - r["max1"][None]) / r["max1"][None], np.abs(r["err2"] - r["max2"][None]) / r["max2"][None])
    return np.where(np.isnan(d), np.inf, d)


def first_success(count, n_its, min_inliers=MIN_INLIERS):
    """1-based index of the first of the n_its hypotheses with more than min_inliers inliers, 0 = none"""
    hit = np.nonzero(np.asarray(count[:n_its]) > min_inliers)[0]
    return int(hit[0]) + 1 if len(hit) else 0


def serial_loop(count, n_its, min_inliers=MIN_INLIERS):
    """iterate()'s loop as written, :158-201, with the `>= mnBestInliers` bookkeeping of :183-199, over the given counts"""
    best = 0
    for it in range(n_its):
        if count[it] >= best:
            best = count[it]
            if count[it] > min_inliers:
                return it + 1
    return 0


def iterations(n, prob=0.99, min_inliers=MIN_INLIERS, max_its=300):
    """SetRansacParameters, :114-138, written out independently of the library's helper; None where iterate() bails (:146-150)"""
    if n < min_inliers:
        return None
    if n == min_inliers:
        k = 1
    else:
        eps = f32(f32(min_inliers) / f32(n))
        k = int(np.ceil(np.log(1 - prob) / np.log(1 - float(eps) ** 3)))
    return max(1, min(k, max_its))


# ---- fixtures -----------------------------------------------------------------------------------------------------------
NOISE = 0.004                                                  # metres on both point sets: about half a pixel at these depths
CAM_A = np.array([535.4, 539.2, 320.1, 247.6], f32)
CAM_B = np.array([517.3, 516.5, 318.6, 255.3], f32)


def _rot(rng, angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return _rodrigues((ax * angle)[None])[0]


def _draw(n, its, rng):
    """draw-and-swap-with-back, :163-177 (the library's helper is tested against the same property, not used here)"""
    out = np.zeros((its, 3), np.int32)
    for h in range(its):
        avail = list(range(n))
        for i in range(3):
            r = int(rng.integers(0, len(avail)))
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def make_candidate(seed, n, kind, n_its, fix_scale, n_trip=None, swap=False):
    """kind: 'planted' (a true Sim3, 4 mm noise on both point sets -- about half a pixel --, three pairs in ten unrelated), 'exact'
    (no noise, no outliers), 'outliers' (no pair related).  n_its None: the formula's value.  n_trip: triples drawn (default n_its)."""
    rng = np.random.default_rng(7000 * seed + n)
    K1, K2 = (CAM_B, CAM_A) if swap else (CAM_A, CAM_B)
    R, t = _rot(rng, 0.3), rng.normal(size=3) * 0.4
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    box = lambda m: np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1.1, 1.1, m), rng.uniform(3.0, 8.0, m)], -1)
    X2 = box(n)
    X1 = s * X2 @ R.T + t
    if kind == "planted":
        X1 += NOISE * rng.normal(size=(n, 3))
        X2 = X2 + NOISE * rng.normal(size=(n, 3))
        bad = rng.uniform(size=n) < 0.3
        X1[bad] = box(int(bad.sum()))
    elif kind == "outliers":
        X1 = box(n)
    lvl = lambda: (f32(1.2) ** rng.integers(0, 4, n).astype(f32)) ** 2
    if n_its is None:
        n_its = iterations(n) or 0
    n_trip = n_its if n_trip is None else n_trip
    tri = _draw(n, n_trip, rng) if n >= 3 else np.zeros((0, 3), np.int32)
    return dict(K1=K1.copy(), K2=K2.copy(), X1c=X1.astype(f32), X2c=X2.astype(f32), sigma2_1=lvl().astype(f32), sigma2_2=lvl().astype(f32),
                triples=tri, n_its=min(n_its, len(tri)), true=dict(R=R, t=t, s=s), kind=kind)


def degenerate_candidate(seed, fix_scale):
    """65 planted matches whose first six are rewritten: 0, 1, 2 the same pair three times, at coordinates whose float32 sums are exact
    (coincident points: centroid = point in both flavours, M = 0, N = 0, the first eigenvector is (1,0,0,0), norm(vec) = 0); 3, 4, 5 on lines parallel to the optical axis in both cameras, in the same
    order, at coordinates float32 sums keep exact (N = diag(c, -c, -c, c) with c > 0 exactly: no rotation, the tie goes to the
    first, norm(vec) = 0 again).  Collinear points in general leave a two-dimensional eigenspace, and which of its vectors a solver
    returns -- a turn by pi about the line is in it -- is not defined; only this line is a fixture.  Triples 0 and 1 are those two;
    four ordinary ones follow."""
    c = make_candidate(seed, 65, "planted", 6, fix_scale)
    c["X1c"][0:3] = (0.75, -0.5, 4.0)
    c["X2c"][0:3] = (0.5, 0.25, 5.0)
    for k, (z1, z2) in enumerate(((3.0, 4.0), (4.0, 5.5), (5.5, 7.5))):
        c["X1c"][3 + k] = (0.25, 0.5, z1)
        c["X2c"][3 + k] = (0.5, -0.25, z2)
    c["triples"][0] = (0, 1, 2)
    c["triples"][1] = (3, 4, 5)
    c["kind"] = "degenerate"
    return c


def z0_candidate(seed, fix_scale):
    """64 planted matches; match 7 has z = 0 in camera 1 and match 9 in camera 2 (p = inf or NaN: an outlier under every
    hypothesis); the first two of its five triples contain them"""
    c = make_candidate(seed, 64, "planted", 5, fix_scale, swap=True)
    c["X1c"][7, 2] = 0.0
    c["X2c"][9, 2] = 0.0
    c["triples"][0] = (7, 20, 30)
    c["triples"][1] = (9, 11, 40)
    c["kind"] = "z0"
    return c


# (matches, kind, n_its (None: the formula), triples drawn (None: n_its), seed): wave edges (63, 64, 65), a third stride pass (129),
# the staged / unstaged threshold of the kernel (256 matches: 300 reads global memory), N below, at and just above minInliers, no
# matches, no iterations with triples present, fewer iterations than triples, pure outliers, success at iteration 1 (21 exact
# pairs).  The seeds are the first for which the restatement ALONE meets the conditions tests/test_oracle_sim3_ransac.py asserts.
POOL = [(0, "planted", 0, None, 1), (3, "planted", 1, None, 1), (19, "planted", 5, None, 1), (20, "exact", None, None, 1),
        (21, "exact", None, None, 1), (63, "planted", None, None, 1), (64, "planted", None, None, 1), (65, "planted", None, None, 1),
        (129, "planted", None, None, 1), (300, "planted", None, None, 1), (100, "outliers", 300, None, 1), "degenerate", "z0",
        (129, "planted", 0, 5, 2), (300, "planted", 6, 9, 2), (21, "planted", 1, None, 1), (63, "planted", 5, None, 2)]
SEED_DEGENERATE, SEED_Z0 = 1, 1
BATCH3 = [9, 11, 5]


@functools.lru_cache(maxsize=None)
def pool(fix_scale):
    """the 17 candidates of one fix_scale setting (inputs only; treat as read-only)"""
    out = []
    for i, p in enumerate(POOL):
        if p == "degenerate":
            out.append(degenerate_candidate(SEED_DEGENERATE, fix_scale))
        elif p == "z0":
            out.append(z0_candidate(SEED_Z0, fix_scale))
        else:
            n, kind, n_its, n_trip, seed = p
            out.append(make_candidate(seed, n, kind, n_its, fix_scale, n_trip, swap=bool(i & 1)))
    return out


@functools.lru_cache(maxsize=None)
def pool_results(fix_scale, flavour):
    return [evaluate(c, fix_scale, flavour) for c in pool(fix_scale)]


@functools.lru_cache(maxsize=None)
def measured():
    """CPU: over every fixture, the smallest band outside which the "f32" flavour's flags equal the "f64" flavour's (the largest
    knife-edge distance of a pair they disagree on)"""
    band = 0.0
    for fix in (0, 1):
        for a, b in zip(pool_results(fix, "f32"), pool_results(fix, "f64")):
            diff = a["flags"] != b["flags"]
            if diff.any():
                band = max(band, float(edge(b)[diff].max()))
    return band


def band():
    """what tests/test_gpu_sim3_ransac.py leaves undecided: 4 x the measured band"""
    return 4 * measured()


def flavour_distance(fix_scale, i, h):
    """the "f32" flavour's own distance to "f64" in R, t, s of hypothesis h of candidate i: what the reference's float32 arithmetic
    is worth on THAT transform (a maximum over all hypotheses would be set by the worst-conditioned junk triple)"""
    a, b = pool_results(fix_scale, "f32")[i], pool_results(fix_scale, "f64")[i]
    return {k: float(np.abs(np.asarray(a[k][h], f64) - b[k][h]).max()) for k in ("R", "t", "s")}


def in_band_fraction(r64, n_its, width):
    """share of the (hypothesis, match) pairs of a candidate's first n_its hypotheses inside the band, and their number"""
    e = edge(r64)[:n_its]
    return (float((e < width).mean()) if e.size else 0.0), int((e < width).sum())


def count_interval(r64, width):
    """per hypothesis: the sure-inlier count and sure plus in-band"""
    e = edge(r64)
    sure = (r64["flags"] & (e >= width)).sum(1)
    return sure, sure + (e < width).sum(1)


MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sim3_ransac_margins.json")
