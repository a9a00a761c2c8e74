"""The block-row regimes of the dense solve of the bundle adjustment's reduced system (csrc/dense_chol.hpp: k_chol_first / k_chol_step,
k_chol_solve; csrc/ba_solver.hip: k_chol_back), one scene per regime, each the smallest that reaches it.  Shared by
tests/test_oracle_ba_blocks.py (the C oracle on the CPU: is every scene what the table says, and how sharp is the reference there?) and tests/test_gpu_ba_blocks.py
(the device solve against that oracle).  Nothing here touches a GPU.

The solver works on 64-wide block rows, nb = dimp / 64, dimp = the dense dimension padded to a multiple of 64.  The dense dimension
is 6 x (free key-frames) with the objects eliminated in front of the solve (the default) and 6 x (free key-frames + active objects)
with the objects inside it.  What changes with nb:

    nb = 1            one block: k_chol_first alone, also on a problem set up for the chain form
    nb = 2            the chain workgroup alone (no tile workgroup below three block rows)
    nb >= 3           tile workgroups beside the chain, nb (nb - 1) / 2 tiles
    nb >= 6           the split back-substitution deals 4 j units of step j over 16 waves: a wave takes a second unit
    nb >= 18          the wave-strided loops over block rows (k = wave, wave + 16, ..) wrap
    tiles > n_cu - 1  a tile workgroup takes a second ticket (nb >= 24 on 256 compute units)
    dimp <= 1984      the split form of k_chol_back: y, x and 8 partial sums per row, 8 (10 dimp + 64) bytes of the 160 KiB of LDS
    dimp >= 2048      its other form (whole blocks per wave)
    dim == dimp       no padding row: the identity tail of k_schur_prepare is empty and the eliminated objects' slots of x start
                      right at dimp.  6 n is a multiple of 64 when the number of free key-frames is a multiple of 32."""
import collections
import functools

import numpy as np

from qsp_slam_amd import synth

NB = 64                               # block row width of the dense solve
LDS_MAX = 160 * 1024                  # bytes of LDS of a workgroup (SCHUR_ROW_LDS_MAX)
SEED = 23
N_OBJ = 3
NB_TICKET_CAP = 31                    # the ticket scene stays on the split form of the back-substitution
N_CU_CPU = 256                        # the compute-unit count the CPU test derives `b_ticket` for

DM = float(np.float32(np.sqrt(5.991)))      # the Huber deltas of tests/test_gpu_ba.py
DS = float(np.float32(np.sqrt(7.815)))
DO = float(np.float32(np.sqrt(1e3)))

Shape = collections.namedtuple("Shape", "dim dimp nb pad split")


def shape(n_free, n_obj_active, elim):
    """the dense system of `n_free` free key-frames and `n_obj_active` objects -> Shape(dim, dimp, nb, padding rows, split form?)"""
    dim = 6 * (n_free + (0 if elim else n_obj_active))
    dimp = (dim + NB - 1) // NB * NB
    return Shape(dim, dimp, dimp // NB, dimp - dim, 8 * (10 * dimp + NB) <= LDS_MAX)


def ticket_nb(n_cu):
    """the smallest nb at which nb (nb - 1) / 2 tiles exceed the n_cu - 1 tile workgroups of a launch, at most NB_TICKET_CAP
    -> (nb, True when the cap applied)"""
    nb = 3
    while nb * (nb - 1) // 2 <= n_cu - 1 and nb < NB_TICKET_CAP:
        nb += 1
    return nb, nb * (nb - 1) // 2 <= n_cu - 1


# name -> (key-frames, landmarks, (dim, dimp) with the objects eliminated, (dim, dimp) with the objects inside, regime).  One key-frame
# of a scene is fixed; a landmark has 8 observations, so a key-frame has 8 n_pt / n_kf of them (48 or more).
TABLE = collections.OrderedDict([
    ("b1",        (11,  300,  (60, 64),     (78, 128),    "one block, 4 padding rows")),
    ("b2",        (12,  300,  (66, 128),    (84, 128),    "the chain alone, no tile")),
    ("b3_exact",  (33,  300,  (192, 192),   (210, 256),   "first tiles; no padding")),
    ("b4_pad",    (34,  300,  (198, 256),   (216, 256),   "58 padding rows")),
    ("b6_exact",  (65,  400,  (384, 384),   (402, 448),   "second unit pass of the split back-substitution")),
    ("b18_exact", (193, 1200, (1152, 1152), (1170, 1216), "the wave-strided loops wrap")),
    ("b_ticket",  None),              # derived from the compute-unit count, see entry()
    ("b31",       (331, 2000, (1980, 1984), (1998, 2048), "last split size")),
    ("b32",       (342, 2100, (2046, 2048), (2064, 2112), "first size of the other form")),
])
NAMES = list(TABLE)
DENSE_ORACLE = NAMES[: NAMES.index("b18_exact") + 1]      # the oracle's dense solver takes 26 s at b32: only up to here
ATOMIC = ["b3_exact", "b6_exact", "b32"]


def entry(name, n_cu=N_CU_CPU):
    """-> dict(n_kf, n_pt, elim=(dim, dimp), joint=(dim, dimp), regime)"""
    if name != "b_ticket":
        n_kf, n_pt, e, j, regime = TABLE[name]
        return dict(n_kf=n_kf, n_pt=n_pt, elim=e, joint=j, regime=regime)
    nb, capped = ticket_nb(n_cu)
    n_free = NB * nb // 6                                   # the most key-frames in nb block rows (exact when nb is a multiple of 3)
    regime = "a tile workgroup takes a second ticket (%d tiles, %d compute units)" % (nb * (nb - 1) // 2, n_cu)
    if capped:
        regime = "capped at %d block rows: %d tiles do not exceed %d compute units" % (nb, nb * (nb - 1) // 2, n_cu)
    e, j = shape(n_free, N_OBJ, True), shape(n_free, N_OBJ, False)
    return dict(n_kf=n_free + 1, n_pt=max(300, 6 * (n_free + 1)), elim=(e.dim, e.dimp), joint=(j.dim, j.dimp), regime=regime)


@functools.lru_cache(maxsize=None)
def scene(name, n_cu=N_CU_CPU):
    """built once per session; nobody writes into it (both problem classes copy what they keep)"""
    e = entry(name, n_cu)
    return synth.make_ba_scene_large(SEED, e["n_kf"], e["n_pt"], obs_per_pt=8, n_obj=N_OBJ)


def rel(a, b, rtol, atol):
    """the effective relative error of np.allclose(a, b, rtol, atol): max |a - b| / (|b| + atol / rtol)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + atol / rtol)).max()) if a.size else 0.0
