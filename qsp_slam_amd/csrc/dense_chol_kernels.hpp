// dense_chol_kernels.hpp -- the definitions behind dense_chol.hpp.  Included by ba_solver.hip only: one object defines the
// kernels, the others launch them through the declarations.
#pragma once
#include <stdint.h>

#include "dense_chol.hpp"

namespace qsp {
namespace ba {

// ---------------------------------------------------------------------------------------------------------------
// Dense SPD solve of the reduced system  Hs x = bs  (dimp multiple of NB = 64), replacing g2o's LDLT
// (linear_solver_eigen.h:94-124).  Right-looking blocked Cholesky Hs = L L^T with ONE launch per block step:
//   * workgroup (i,j), k < i <= j, forms the two panel blocks it needs itself, P_i = L_kk^-1 A_ki and P_j = L_kk^-1 A_kj,
//     as products with the explicit inverse W_k = L_kk^-1 (no triangular solves anywhere), and updates A_ij -= P_i^T P_j;
//   * the first row of workgroups (i = k+1) also stores P_j as the factor's block row k and carries the right-hand side
//     along (forward substitution comes for free: y_k = W_k b_k, b_j -= P_j^T y_k);
//   * workgroup (k+1,k+1) goes on to factorise its freshly updated diagonal block in registers -- Gauss steps applied
//     to [S | I] give L^-1 beside the factor -- so the next launch finds W_{k+1} and y_{k+1} ready.
// The backward substitution x_k = W_k^T (y_k - sum_j U_kj x_j) is nb small launches of matrix-vector products.
// ---------------------------------------------------------------------------------------------------------------
static_assert(NB * (NB + 1) <= 2 * NB * NB, "Wr (NB x 65) lies over X and the head of Yi");

// The 64x64x64 products of the factorisation on the FP64 matrix pipe: wave w of four forms rows 16w..16w+15 of the result as
// four 16x16 tiles, acc[tc] (+)= sum_m A(m, 16w + i) B[m][16 tc + j] with A(m, r) = X[m sk + r si] (so the left operand may be
// stored either way round, with any pitch) and B row-major with pitch NB.  v_mfma_f64_16x16x4_f64: lane l carries A[i = l & 15]
// [k = l >> 4] and B[k = l >> 4][j = l & 15]; its four results are rows (l >> 4) + 4 reg, column l & 15 of the tile.  The matrix
// pipe's FP64 rate equals the vector pipe's on this part; what it saves is LDS traffic -- one operand double per lane and 1024
// multiply-adds against eight doubles per 16 with 4x4 register tiles, which kept the four waves of a compute unit waiting on the
// LDS for ~60 % of a product (10.5 k cycles per product measured, 4.1 k of arithmetic).
typedef double d4_t __attribute__((ext_vector_type(4)));
__device__ inline void mfma_gemm64(const double* X, int sk, int si, const double* B, int wave, int lane, d4_t (&acc)[4]) {
    const double* xa = X + (lane >> 4) * sk + (16 * wave + (lane & 15)) * si;
    const double* yb = B + (lane >> 4) * NB + (lane & 15);
#pragma unroll 4
    for (int ks = 0; ks < NB / 4; ++ks) {
        const double a = xa[4 * ks * sk];
#pragma unroll
        for (int tc = 0; tc < 4; ++tc) acc[tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[4 * ks * NB + 16 * tc], acc[tc], 0, 0, 0);
    }
}
// the wave's four result tiles into a row-major 64x64 LDS image
__device__ inline void mfma_store64(double* Z, const d4_t (&acc)[4], int wave, int lane) {
#pragma unroll
    for (int tc = 0; tc < 4; ++tc)
#pragma unroll
        for (int r = 0; r < 4; ++r) Z[(16 * wave + (lane >> 4) + 4 * r) * NB + 16 * tc + (lane & 15)] = acc[tc][r];
}
// the factor's block U_kj = P (64 x 64) goes to memory TRANSPOSED, element (m, c) at Uf[(j NB + c) ld + k NB + m]: the backward
// substitution walks it by rows m with a lane per row.  Straight from the result registers (4 consecutive m per 16 lanes).
__device__ inline void mfma_store_factor(double* Uf, int ld, int j, int k, const d4_t (&acc)[4], int wave, int lane) {
#pragma unroll
    for (int tc = 0; tc < 4; ++tc)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            Uf[(size_t)(j * NB + 16 * tc + (lane & 15)) * ld + k * NB + 16 * wave + (lane >> 4) + 4 * r] = acc[tc][r];
}

// 1/sqrt(d): hardware estimate + two Newton steps (full double precision to an ulp or two; keeps the f64 divide and
// square-root sequences off the factorisation's serial chain)
__device__ inline double rsqrt_nr(double d) {
    double r = __builtin_amdgcn_rsq(d);
    r = r * (1.5 - 0.5 * d * r * r);
    r = r * (1.5 - 0.5 * d * r * r);
    return r;
}

// Factorisation of a 64x64 SPD block by 320 threads: four UPDATER waves hold S (and W = L^-1, grown from the identity by the same
// row operations) as 4x4 register tiles (thread owns rows r0.., cols c0..); a fifth PANEL wave (lane = column) owns the serial
// chain.  Phase p (one workgroup barrier each):
//   panel     takes rows 4p..4p+3 of [S | W] as the updaters left them one block earlier (nx), applies block p-1 itself (8 values
//             per lane), fetches the 4x4 diagonal values by v_readlane, factorises them (Newton rsqrt), finishes its column of
//             the four rows of U and W and publishes them (rb; the W rows also into Wr, pitch 65, for the tail);
//   updaters  apply block p-1 (rank 4) to every tile below it; the 16 threads owning rows 4(p+1).. then hand their tiles to the
//             panel wave (nx) for the next phase.
// The pivot chain and the rank-4 update overlap instead of alternating: 14.1 against 20.6 us per block on MI355X
// (tools/micro/chol_factor.hip, variants 0 and 5), every element going through the same operations in the same order (the two
// forms agree in every bit).  S is consumed.  rowbuf: CHOL_ROWBUF doubles of LDS (rb and nx, double-buffered); Wr: NB x 65.
// From phase FETCH_PHASE on the first two updater waves have no rows left (rows 0..31 are final): k_chol_chain gives them another
// job there -- fetching the next step's tiles (Fetch::phase(p), once per phase) -- in a loop of their own, so that what they keep
// in registers does not weigh on the loops of the waves still at work.
// (the phases exchange data through LDS only: their barrier waits for this wave's LDS traffic, not for global loads the fetching
//  waves have in flight across them)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
constexpr int FETCH_PHASE = NB / 8;
struct NoFetch {
    static constexpr bool active = false;
    struct Regs {};
    __device__ __forceinline__ void phase(int, Regs&) const {}
    __device__ __forceinline__ void finish(Regs&) const {}
};

struct FactorLds { double *rbuf, *nx, *Wr; };
// what the panel wave carries from phase p-1 into phase p: its own column of the block it has just published (U and W rows) and
// that block's entries in columns 4p..4p+3 -- the latter read back from LDS right behind the stores, in FRONT of the barrier, so
// that behind it only the rows handed over by the updaters remain to be fetched
struct PanelCarry { double s[4], w[4], ur[4][4]; };
// the panel wave's phase p; returns whether a pivot was not positive
__device__ __forceinline__ bool factor_panel_phase(int p, const FactorLds& L, int lane, PanelCarry& pc) {
    bool bad = false;
    double* rb = L.rbuf + (p & 1) * 8 * NB;
    const double* in = L.nx + (p & 1) * 8 * NB;
    double s[4], w[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { s[a] = in[a * NB + lane]; w[a] = in[(4 + a) * NB + lane]; }
    if (p > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                s[a] -= pc.ur[q][a] * pc.s[q];
                w[a] -= pc.ur[q][a] * pc.w[q];
            }
        }
    }
    double D[4][4], rs[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {      // (a uniform lane index: v_readlane to scalar registers, no LDS round trip)
            union { double d; int i[2]; } u, r;
            u.d = s[a];
            r.i[0] = __builtin_amdgcn_readlane(u.i[0], 4 * p + b);
            r.i[1] = __builtin_amdgcn_readlane(u.i[1], 4 * p + b);
            D[a][b] = r.d;
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double dd = D[q][q];
        const bool isbad = !(dd > 0) || !isfinite(dd);
        bad |= isbad;
        if (isbad) dd = 1.0;
        rs[q] = rsqrt_nr(dd);
#pragma unroll
        for (int b = q + 1; b < 4; ++b) D[q][b] *= rs[q];
#pragma unroll
        for (int a = q + 1; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b) D[a][b] -= D[q][a] * D[q][b];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double sv = s[q], wv = w[q];
#pragma unroll
        for (int pp = 0; pp < q; ++pp) { sv -= D[pp][q] * s[pp]; wv -= D[pp][q] * w[pp]; }
        s[q] = sv * rs[q];
        w[q] = wv * rs[q];
        rb[q * NB + lane] = s[q];
        rb[(4 + q) * NB + lane] = w[q];
        L.Wr[(4 * p + q) * (NB + 1) + lane] = w[q];
        pc.s[q] = s[q];
        pc.w[q] = w[q];
    }
    if (p + 1 < NB / 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a) pc.ur[q][a] = rb[q * NB + 4 * (p + 1) + a];     // (this wave's own stores: LDS keeps their order)
    }
    return bad;
}
// an updater thread's phase p
__device__ __forceinline__ void factor_updater_phase(int p, const FactorLds& L, double (&S)[4][4], double (&W)[4][4], int r0, int c0) {
    const double* rbp = L.rbuf + ((p + 1) & 1) * 8 * NB;       // block p-1
    if (p > 0 && r0 > 4 * (p - 1)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double ur[4], uc[4], wc[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { ur[a] = rbp[q * NB + r0 + a]; uc[a] = rbp[q * NB + c0 + a]; wc[a] = rbp[(4 + q) * NB + c0 + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) { S[a][b] -= ur[a] * uc[b]; W[a][b] -= ur[a] * wc[b]; }
        }
    }
    if (r0 == 4 * (p + 1)) {
        double* out = L.nx + ((p + 1) & 1) * 8 * NB;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) { out[a * NB + c0 + b] = S[a][b]; out[(4 + a) * NB + c0 + b] = W[a][b]; }
    }
}

template <class Fetch>
__device__ __forceinline__ bool factor_tile64(double (&S)[4][4], double* Wr, double* rowbuf, int r0, int c0, Fetch& fetch) {
    bool bad = false;
    const int t = threadIdx.x, lane = t & 63;
    const bool panel = t >= 256;
    const FactorLds L{rowbuf, rowbuf + 2 * 8 * NB, Wr};
    double W[4][4];
    if (!panel) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) W[a][b] = (r0 + a == c0 + b) ? 1.0 : 0.0;
        if (r0 == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) { L.nx[a * NB + c0 + b] = S[a][b]; L.nx[(4 + a) * NB + c0 + b] = W[a][b]; }
        }
    }
    lds_barrier();
    if (panel) {
        __builtin_amdgcn_s_setprio(3);              // (it shares a SIMD with an updater wave and everybody waits for it)
        PanelCarry pc;
#pragma nounroll
        for (int p = 0; p < NB / 4; ++p) {
            bad |= factor_panel_phase(p, L, lane, pc);
            lds_barrier();
        }
        __builtin_amdgcn_s_setprio(0);
    } else {
#pragma nounroll
        for (int p = 0; p < FETCH_PHASE; ++p) {
            factor_updater_phase(p, L, S, W, r0, c0);
            lds_barrier();
        }
        if (Fetch::active && t < 128) {
            typename Fetch::Regs regs;               // (what is in flight lives in this loop only)
#pragma nounroll
            for (int p = FETCH_PHASE; p < NB / 4; ++p) {
                fetch.phase(p, regs);
                lds_barrier();
            }
            fetch.finish(regs);
        } else {
#pragma nounroll
            for (int p = FETCH_PHASE; p < NB / 4; ++p) {
                factor_updater_phase(p, L, S, W, r0, c0);
                lds_barrier();
            }
        }
    }
    return bad;
}

// tail shared by the first launch and workgroup (k+1,k+1), 320 threads: factorise block kb, publish W_kb^T and y_kb = W_kb b_kb.
// bvec (LDS, NB doubles) holds the fully updated right-hand-side block; Wr (LDS, NB x 65) receives the rows of W.
__device__ inline void factor_and_forward(double (&S)[4][4], int kb, double* Winv, double* y, double* Wr, double* rowbuf,
                                          const double* bvec, double* scal, int r0, int c0) {
    NoFetch nofetch;
    const bool bad = factor_tile64(S, Wr, rowbuf, r0, c0, nofetch);
    if (bad) scal[3] = 1.0;                                        // (the panel wave's lanes: one value, 64 writers)
    // (the loop's last barrier has made Wr complete.)  W^T to global: WT[m][q] = W[q][m]
    double* Wg = Winv + (size_t)kb * NB * NB;
    for (int e = threadIdx.x; e < NB * NB; e += CHOL_THREADS) Wg[e] = Wr[(e % NB) * (NB + 1) + e / NB];
    if (threadIdx.x < NB) {
        double v = 0;
        for (int m = 0; m < NB; ++m) v += Wr[threadIdx.x * (NB + 1) + m] * bvec[m];
        y[kb * NB + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(CHOL_THREADS) void k_chol_first(const double* A, double* Winv, const double* b, double* y, int ld,
                                                             double* scal) {
    extern __shared__ __attribute__((aligned(16))) double chol_lds[];
    double* X = chol_lds;
    double* rowbuf = chol_lds + 3 * NB * NB;
    double* bvec = rowbuf + CHOL_ROWBUF;
    const int t = threadIdx.x, r0 = (t >> 4) * 4, c0 = (t & 15) * 4;
    double S[4][4];
    if (t < 256) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[a][q] = A[(size_t)(r0 + a) * ld + c0 + q];
    }
    if (t < NB) bvec[t] = b[t];
    __syncthreads();
    factor_and_forward(S, 0, Winv, y, X, rowbuf, bvec, scal, r0, c0);
}

// grid (n, n), n = nb - k - 1: x = j - k - 1, y = i - k - 1; workgroups below the diagonal leave at once.  320 threads: the
// fifth wave is factor_tile64's panel wave and has work in workgroup (k+1,k+1) only (there it also carries the right-hand side
// while the others are in the second product).
__global__ __launch_bounds__(CHOL_THREADS) void k_chol_step(double* A, double* Uf, double* Winv, double* b, double* y, int ld, int k,
                                                            double* scal) {
    const int j = k + 1 + blockIdx.x, i = k + 1 + blockIdx.y;
    if (i > j) return;
    const int t = threadIdx.x, r0 = (t >> 4) * 4, c0 = (t & 15) * 4;
    const bool first_row = (i == k + 1);
    const bool chain = first_row && i == j;               // this workgroup goes on to factorise block k+1
    const bool upd = t < 256;                             // (elsewhere the fifth wave only walks through the barriers)
    extern __shared__ __attribute__((aligned(16))) double chol_lds[];
    double* X = chol_lds;
    double* Yi = chol_lds + NB * NB;
    double* Yj = (i == j) ? Yi : chol_lds + 2 * NB * NB;
    double* rowbuf = chol_lds + 3 * NB * NB;
    double* bvec = rowbuf + CHOL_ROWBUF;
    const double* Wg = Winv + (size_t)k * NB * NB;
    double S[4][4];                                       // the tile this thread updates: in flight behind the panel loads
    if (upd) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[a][q] = A[(size_t)(i * NB + r0 + a) * ld + j * NB + c0 + q];
        for (int e = t; e < NB * NB; e += 256) {
            X[e] = Wg[e];
            Yi[e] = A[(size_t)(k * NB + e / NB) * ld + i * NB + e % NB];
            if (i != j) Yj[e] = A[(size_t)(k * NB + e / NB) * ld + j * NB + e % NB];
        }
    }
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    d4_t pi[4] = {}, pj[4] = {};
    if (upd) {
        mfma_gemm64(X, NB, 1, Yi, wave, lane, pi);
        if (i != j) mfma_gemm64(X, NB, 1, Yj, wave, lane, pj);
    }
    __syncthreads();
    if (upd) {
        mfma_store64(Yi, pi, wave, lane);
        if (i != j) mfma_store64(Yj, pj, wave, lane);
    }
    __syncthreads();
    if (upd) {
        d4_t acc[4] = {};
        mfma_gemm64(Yi, NB, 1, Yj, wave, lane, acc);
        mfma_store64(X, acc, wave, lane);          // (X is free since the first products: the way back to the 4x4 register tiles)
    }
    __syncthreads();
    if (upd) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[a][q] -= X[(r0 + a) * NB + c0 + q];
    }
    if (first_row) {
        if (upd) {
            if (i == j) mfma_store_factor(Uf, ld, j, k, pi, wave, lane);
            else mfma_store_factor(Uf, ld, j, k, pj, wave, lane);
        }
        // b_j -= P_j^T y_k: by the panel wave where there is one (beside the second product), by the first wave elsewhere
        const int tb = chain ? t - 256 : t;
        if (tb >= 0 && tb < NB) {
            double v = b[j * NB + tb];
            for (int q = 0; q < NB; ++q) v -= Yj[q * NB + tb] * y[k * NB + q];
            b[j * NB + tb] = v;
            bvec[tb] = v;
        }
    }
    if (chain) {
        __syncthreads();
        factor_and_forward(S, k + 1, Winv, y, X, rowbuf, bvec, scal, r0, c0);
    } else if (upd) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) A[(size_t)(i * NB + r0 + a) * ld + j * NB + c0 + q] = S[a][q];
    }
}

// ---- the same factorisation as ONE launch: a resident chain workgroup and tile workgroups beside it (k_chol_solve) ----
// k_chol_step pays a kernel boundary on the serial chain of every step: kernel start, the reload of W_k and of two tiles another
// compute unit has just written, the drain of its own stores (~13 of a step's 31 us at C5).  Here the chain -- update of the next
// diagonal tile, its factorisation, y_k -- stays in one workgroup that never leaves its compute unit (chol_chain_body; W_k is used
// where factor_tile64 left it in LDS), and every other tile is taken by a workgroup that keeps it in registers through all its
// steps (chol_trail_tile).  They meet through epoch-valued flags in global memory (no reset between solves):
//   flag_w[k]         set by the chain once W_k^T and y_k are in global memory   -> awaited by every tile workgroup at its step k
//   tile_done[i nb+j] set by tile (i,j)'s workgroup once the tile is final in memory (for i = k+1 also: U_kj stored, b_j carried
//                     through step k)   -> awaited by the tiles of later rows that multiply with it and, for (s-1,s) and (s,s),
//                     by the chain before its step s
// Release: stores, workgroup barrier, then one thread's agent-scope fence and flag store; acquire: one thread polls (relaxed,
// agent scope), fences, workgroup barrier.  Every wait is bounded (CHOL_SPIN_MAX polls): on expiry scal[5] is raised, later waits
// give up at once and the kernel runs to its end on whatever it finds: the grid always drains; the host then repeats THAT trial
// on the one-launch-per-step form, which the problem keeps from there on (qsp_ba_optimize).  Every flag a workgroup
// waits for is set by the chain or by a tile of an EARLIER row -- a smaller TICKET, i.e. a workgroup that is running or done
// (k_chol_solve) -- and the chain waits for nothing a step ahead of it, so the scheme cannot wait on itself whichever workgroups
// the dispatcher starts first.  The chain's last steps have (transitively) awaited every tile_done of the solve: when the chain
// workgroup ends, every write of the tile workgroups is complete and visible to the kernels behind it in the stream.
// Same operations in the same order on every element as the k_chol_step path (the two agree in every bit).
#ifdef QSP_CB_STAMPS      // timing experiments only: shader-clock stamps of the chain workgroup's thread 0 at the phase boundaries of every step
__device__ unsigned long long qsp_chain_ts[64 * 8];
#define QSP_CHTS(s_, i_) { if (threadIdx.x == 0 && (s_) < 64) qsp_chain_ts[(s_) * 8 + (i_)] = __builtin_readcyclecounter(); }
#else
#define QSP_CHTS(s_, i_)
#endif
constexpr int CHOL_SPIN_MAX = 1 << 20;      // x (poll + s_sleep) ~ 1-2 us: a second or two
__device__ inline void chol_signal(unsigned* flag, unsigned epoch) {      // call after a workgroup barrier, one thread
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one thread: wait until *flag == epoch.  A wait that expires raises scal[5]; every later wait of the solve gives up at once
// (scal[5] is polled too), so a broken run costs one time-out, not one per step.
__device__ inline void chol_wait3(const unsigned* fa, const unsigned* fb, const unsigned* fc, unsigned epoch, double* scal) {
    const unsigned long long* dead = reinterpret_cast<const unsigned long long*>(scal + 5);
    for (int spin = 0; spin < CHOL_SPIN_MAX; ++spin) {
        // (the looks go out together: one round trip, not one per flag)
        const unsigned a = __hip_atomic_load(fa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned b = fb ? __hip_atomic_load(fb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
        const unsigned c = fc ? __hip_atomic_load(fc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
        if (a == epoch && b == epoch && c == epoch) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            return;
        }
        if ((spin & 255) == 0 && __hip_atomic_load(dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) return;
        __builtin_amdgcn_s_sleep(4);
    }
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(scal + 5), 0x3ff0000000000000ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // 1.0
}
__device__ inline void chol_wait(const unsigned* flag, unsigned epoch, double* scal) { chol_wait3(flag, nullptr, nullptr, epoch, scal); }

// a wave-load of 64 consecutive doubles from a UNIFORM address: scalar base + this lane's 32-bit byte offset (one VGPR of address
// for all loads of the kernel instead of a 64-bit pointer per load in flight)
typedef const __attribute__((address_space(1))) char* gbytes_t;
__device__ __forceinline__ double ld_row(const double* uniform_ptr, uint32_t voff) {
    return *reinterpret_cast<const __attribute__((address_space(1))) double*>((gbytes_t)uniform_ptr + voff);
}

constexpr int CHAIN_PROBE_GAP = 2;        // phases between a look at the flags and reading what it returned
constexpr int CHAIN_PARK_AFTER = 3;       // phases between issuing the next step's loads and parking them in LDS
// Fetching ahead (the first two updater waves in the second half of factor_tile64, 128 threads): thread 0 looks at the two flags
// the next step needs -- two relaxed loads, read CHAIN_PROBE_GAP phases later: they take 1-2 us to come back, a phase 0.8 us, and
// the thread must not sit in front of a phase barrier waiting for them -- and looks again until both are up; then it fences
// (acquire) and raises go[0]; every fetching thread that sees go[0] issues its share of the two tiles (2 x 32 doubles) and, the
// first wave, of b; CHAIN_PARK_AFTER phases later, or behind the last phase, the values are parked in LDS (Sn, Yp, bnext: all free
// during a factorisation).  go[1] = thread 0 has issued its loads (the others have by the
// phase after): read by the whole workgroup at the top of the next step.
struct ChainFetch {
    static constexpr bool active = true;
    const double* A;
    const double* b;
    const unsigned *fa, *fb;       // tile_done of (sn-1, sn) and (sn, sn)
    double *Sn, *Yp, *bnext;
    volatile int* go;
    unsigned epoch, f0, f1;
    int ld, sn, nb, t;
    int st;                        // thread 0: bit 0 a look is in flight, bit 1 flags up;  all: bit 2 loads issued, bit 3 parked
    int p_mark;
    struct Regs { double T[64], b2; };
    __device__ __forceinline__ void issue(int p, Regs& r) {
        // element e = t + 128 i of a tile: row (t >> 6) + 2 i, column t & 63 -- a uniform row base per i and ONE 32-bit offset per
        // thread (64 full addresses in flight would cost the fetching waves 128 registers)
        uint32_t voff = 8u * (uint32_t)((t >> 6) * ld + (t & 63));
        const double* baseS = A + (size_t)(sn * NB) * ld + sn * NB;
        const double* baseY = A + (size_t)((sn - 1) * NB) * ld + sn * NB;
        // (opaque to the optimiser: left alone it forms the 64 addresses in vector registers in front of the phase loop and keeps
        //  them there, 128 registers the loads' results then have to share with)
        asm volatile("" : "+s"(baseS), "+s"(baseY), "+v"(voff));
        const size_t step = (size_t)2 * ld;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            r.T[i] = ld_row(baseS, voff);
            r.T[32 + i] = ld_row(baseY, voff);
            baseS += step;
            baseY += step;
            asm volatile("" : "+s"(baseS), "+s"(baseY));
        }
        if (t < NB) r.b2 = b[sn * NB + t];
        st |= 4;
        p_mark = p;
    }
    __device__ __forceinline__ void park(Regs& r) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            Sn[t + 128 * i] = r.T[i];
            Yp[t + 128 * i] = r.T[32 + i];
        }
        if (t < NB) bnext[t] = r.b2;
        st |= 8;
    }
    // (loads issued in the last phases are parked behind the loop: the fetching waves then wait while the others publish W_s)
    __device__ __forceinline__ void finish(Regs& r) {
        if ((st & 4) && !(st & 8)) park(r);
    }
    __device__ __forceinline__ void phase(int p, Regs& r) {
        if (sn >= nb) return;
        if (st & 4) {
            if (!(st & 8) && p >= p_mark + CHAIN_PARK_AFTER) park(r);
            return;
        }
        if (sn >= 2) {
            if (t == 0 && !(st & 2) && p < NB / 4 - 1) {
                if (!(st & 1)) {
                    f0 = __hip_atomic_load(fa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    f1 = __hip_atomic_load(fb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    st |= 1;
                    p_mark = p;
                } else if (p >= p_mark + CHAIN_PROBE_GAP) {
                    if (f0 == epoch && f1 == epoch) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        go[0] = 1;
                        st |= 2;
                    } else {                        // look again
                        f0 = __hip_atomic_load(fa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        f1 = __hip_atomic_load(fb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        p_mark = p;
                    }
                }
            }
            if (go[0] == 0) return;
        }                                           // (step 1 reads the input itself: fetched at once)
        issue(p, r);
        if (t == 0) go[1] = 1;
    }
};

// One step s of the chain: [tiles (s-1,s), (s,s) and b_s -- normally fetched behind the previous factorisation] ->
// P = W_{s-1} A_{s-1,s} (the panel wave releases W_{s-1} to the tile workgroups meanwhile) -> S -= P^T P, U_{s-1,s} stored,
// b_s -= P^T y_{s-1} (panel wave) -> factor_tile64 -> W_s^T and y_s to memory.
__device__ __forceinline__ void chol_chain_body(double* chol_lds, const double* A, double* Uf, double* Winv, const double* b, double* y, int ld,
                                                int nb, double* scal, unsigned* flag_w, const unsigned* tile_done, unsigned epoch) {
    double* Wr = chol_lds;                          // rows of W_s (pitch 65): factor_tile64 writes them, the next step multiplies with them
    double* Yp = Wr + NB * (NB + 1);                // A_{s-1,s}, then P = W_{s-1} A_{s-1,s}
    double* Sn = Yp + NB * NB;                      // A_{s,s} as the fetching waves park it
    double* rowbuf = Sn + NB * NB;
    double* bvec = rowbuf + CHOL_ROWBUF;
    double* yprev = bvec + NB;
    double* bnext = yprev + NB;                     // b_s as the tile workgroups left it
    int* go_lds = reinterpret_cast<int*>(bnext + NB);
    const int t = threadIdx.x, r0 = (t >> 4) * 4, c0 = (t & 15) * 4;
    const int wave = t >> 6, lane = t & 63;
    const bool upd = t < 256;
    double S[4][4];
    if (upd) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[a][q] = A[(size_t)(r0 + a) * ld + c0 + q];
    }
    if (t < NB) bvec[t] = b[t];
    if (t == 0) go_lds[0] = go_lds[1] = 0;
    ChainFetch f;
    f.A = A; f.b = b; f.Sn = Sn; f.Yp = Yp; f.bnext = bnext; f.go = go_lds; f.epoch = epoch; f.ld = ld; f.nb = nb; f.t = t;
    f.st = 0; f.p_mark = 0; f.f0 = f.f1 = 0; f.sn = nb; f.fa = f.fb = tile_done;
    __syncthreads();
    for (int s = 0; s < nb; ++s) {
        QSP_CHTS(s, 0)
        if (s > 0) {
            // go[1] says for the whole workgroup whether the tiles are on their way: thread 0 issues in the phase in which it raises
            // go[0], every other fetching thread by the phase after, and go[0] is not raised in the last phase
            const bool have = go_lds[1] != 0;
            if (!have) {
                if (s >= 2) {                       // tiles (s-1,s) and (s,s) and b_s as their workgroups leave them
                    if (t == 0) {
                        chol_wait3(tile_done + (s - 1) * nb + s, tile_done + s * nb + s, nullptr, epoch, scal);
                    }
                    __syncthreads();
                }
                if (t < 128) {
                    ChainFetch::Regs r;
                    f.issue(0, r);
                    f.park(r);
                }
            }
            __syncthreads();                        // (everybody has read go[1]; Sn, Yp, bnext complete)
            QSP_CHTS(s, 1)
            if (upd) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int q = 0; q < 4; ++q) S[a][q] = Sn[(r0 + a) * NB + c0 + q];
            }
            if (t == 0) go_lds[0] = go_lds[1] = 0;
            QSP_CHTS(s, 2)
            // W_{s-1}^T and y_{s-1} have been in memory since the barrier that ended step s-1: released here, by the panel wave,
            // which has nothing else to do during the first product (the fence costs 1-2 k cycles)
            if (t == 256) chol_signal(flag_w + s - 1, epoch);
            d4_t pi[4] = {};
            if (upd) mfma_gemm64(Wr, 1, NB + 1, Yp, wave, lane, pi);      // P = W_{s-1} A_{s-1,s}: W's rows as factor_tile64 left them
            lds_barrier();                          // (LDS-only barriers inside a step: nobody waits for the stores of U here)
            QSP_CHTS(s, 3)
            if (upd) mfma_store64(Yp, pi, wave, lane);
            lds_barrier();
            if (upd) {
                d4_t acc[4] = {};
                mfma_gemm64(Yp, NB, 1, Yp, wave, lane, acc);
                mfma_store64(Wr, acc, wave, lane);      // (W_{s-1} has done its work; a plain 64x64 image: the way back to the 4x4 tiles)
                // the factor's block U_{s-1,s} = P, transposed (the tile workgroups of row s store the others)
                mfma_store_factor(Uf, ld, s, s - 1, pi, wave, lane);
            } else {                                // the panel wave, beside the second product: b_s -= P^T y_{s-1}
                double v = bnext[lane];
#pragma unroll 8
                for (int q = 0; q < NB; ++q) v -= Yp[q * NB + lane] * yprev[q];
                bvec[lane] = v;
            }
            lds_barrier();
            if (upd) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int q = 0; q < 4; ++q) S[a][q] -= Wr[(r0 + a) * NB + c0 + q];
            }                                       // (factor_tile64 writes W_s over the image behind its first barrier)
        }
        QSP_CHTS(s, 4)
        f.sn = s + 1;                               // the step to fetch for
        f.st = 0;
        f.fa = tile_done + (size_t)s * nb + s + 1;
        f.fb = tile_done + (size_t)(s + 1) * nb + s + 1;
        const bool bad = factor_tile64(S, Wr, rowbuf, r0, c0, f);
        if (bad) scal[3] = 1.0;
        QSP_CHTS(s, 5)
        double* Wg = Winv + (size_t)s * NB * NB;
        for (int e = t; e < NB * NB; e += CHOL_THREADS) Wg[e] = Wr[(e % NB) * (NB + 1) + e / NB];
        if (t >= 256) {                             // y_s = W_s b_s: the panel wave, a row each
            double v = 0;
            for (int m = 0; m < NB; ++m) v += Wr[lane * (NB + 1) + m] * bvec[m];
            y[s * NB + lane] = v;
            yprev[lane] = v;
        }
        __syncthreads();
        QSP_CHTS(s, 6)
    }
}

// everything off the chain: tile (i,j), 1 <= i <= j < nb, row-major in `tile` -- a tile only ever waits for the chain and for tiles
// of earlier rows, i.e. of SMALLER index.  The tile stays in registers across its steps k = 0 .. i-1 (a diagonal tile leaves its
// last step, k = i-1, to the chain); it goes back to memory once, final, with tile_done(i,j).  256 threads.
__device__ __forceinline__ void chol_trail_tile(double* chol_lds, int tile, double* A, double* Uf, const double* Winv, double* b, const double* y,
                                                int ld, int nb, double* scal, const unsigned* flag_w, unsigned* tile_done, unsigned epoch) {
    {
    int i = 1, rem = tile;
    while (rem >= nb - i) { rem -= nb - i; ++i; }
    const int j = i + rem;
    const int nsteps = (i == j) ? i - 1 : i;
    if (nsteps == 0) return;                          // (tile (1,1): the chain does its only step)
    double* X = chol_lds;
    double* Yi = chol_lds + NB * NB;
    double* Yj = (i == j) ? Yi : chol_lds + 2 * NB * NB;
    double* yk = chol_lds + 3 * NB * NB;
    const int t = threadIdx.x, r0 = (t >> 4) * 4, c0 = (t & 15) * 4;
    double S[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) S[a][q] = A[(size_t)(i * NB + r0 + a) * ld + j * NB + c0 + q];
    for (int k = 0; k < nsteps; ++k) {
        // row k is final once its workgroups have finished (row 0 is the input itself), W_k once the chain has got there: in the
        // steady state all three are up when this workgroup asks (the chain is a step ahead), so one look and ONE batch of loads
        if (t == 0)
            chol_wait3(flag_w + k, k > 0 ? tile_done + k * nb + i : nullptr, (k > 0 && i != j) ? tile_done + k * nb + j : nullptr, epoch, scal);
        __syncthreads();
        const double* Wg = Winv + (size_t)k * NB * NB;
        {
            double vx[16], vi[16], vj[16];            // (all 48 loads of a thread in flight before the first LDS store)
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = t + 256 * u;
                vx[u] = Wg[e];
                vi[u] = A[(size_t)(k * NB + e / NB) * ld + i * NB + e % NB];
                vj[u] = (i != j) ? A[(size_t)(k * NB + e / NB) * ld + j * NB + e % NB] : 0.0;
            }
            if (t < NB) yk[t] = y[k * NB + t];        // (per-lane loads behind the acquire, not a uniform-address scalar load)
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = t + 256 * u;
                X[e] = vx[u];
                Yi[e] = vi[u];
                if (i != j) Yj[e] = vj[u];
            }
        }
        __syncthreads();
        const int wave = t >> 6, lane = t & 63;
        d4_t pi[4] = {}, pj[4] = {};
        mfma_gemm64(X, NB, 1, Yi, wave, lane, pi);
        if (i != j) mfma_gemm64(X, NB, 1, Yj, wave, lane, pj);
        __syncthreads();
        mfma_store64(Yi, pi, wave, lane);
        if (i != j) mfma_store64(Yj, pj, wave, lane);
        __syncthreads();
        {
            d4_t acc[4] = {};
            mfma_gemm64(Yi, NB, 1, Yj, wave, lane, acc);
            mfma_store64(X, acc, wave, lane);        // (X is free since the first products: the way back to the 4x4 register tiles)
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[a][q] -= X[(r0 + a) * NB + c0 + q];
        if (i == k + 1) {                             // (j > i here) the factor's block U_kj and the right-hand side: b_j -= P_j^T y_k
            mfma_store_factor(Uf, ld, j, k, pj, wave, lane);
            if (t < NB) {
                double v = b[j * NB + t];
                for (int q = 0; q < NB; ++q) v -= Yj[q * NB + t] * yk[q];
                b[j * NB + t] = v;
            }
        }
        __syncthreads();                              // (the next step refills X, Yi, Yj, yk)
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) A[(size_t)(i * NB + r0 + a) * ld + j * NB + c0 + q] = S[a][q];
    __syncthreads();
    if (t == 0) chol_signal(tile_done + i * nb + j, epoch);
    }
}

// The factorisation in ONE launch on ONE stream (round 4).  Round 3 ran the chain and the tiles as two kernels on two streams
// that had to be seen running side by side (a handshake per device, an event + a cross-stream wait per solve: 7 us of idle device
// in front of every factorisation, and a way for two problems' stream pairs to block each other when streams share hardware
// queues).  Here every workgroup takes TICKETS from one counter: the first ticket of a solve is the chain, ticket n > 0 is tile
// n - 1.  A ticket is only ever held by a workgroup that is running, a tile waits for the chain and for tiles of smaller index
// only -- smaller tickets, i.e. running or finished workgroups -- so the grid makes progress whichever workgroups the dispatcher
// starts first and however few of them are resident (the blockIdx-strided loop of round 3 lost that guarantee beyond
// 23 block rows).  The counter is never reset: the host passes the value it had before the launch and knows what it will be
// afterwards (every workgroup draws exactly one ticket beyond the solve's range when it leaves).  The chain workgroup has 320
// threads; a workgroup that draws a tile first drops its fifth wave (s_barrier counts the waves that are left).
__global__ __launch_bounds__(CHOL_THREADS) void k_chol_solve(double* A, double* Uf, double* Winv, double* b, double* y, int ld, int nb, double* scal,
                                                             unsigned* flag_w, unsigned* tile_done, unsigned epoch, unsigned* ticket,
                                                             unsigned ticket_base, unsigned n_tiles) {
    extern __shared__ __attribute__((aligned(16))) double chol_lds[];
    __shared__ unsigned s_tk;
    if (threadIdx.x == 0) s_tk = atomicAdd(ticket, 1u) - ticket_base;
    __syncthreads();
    unsigned tk = s_tk;
    if (tk == 0u) {
        chol_chain_body(chol_lds, A, Uf, Winv, b, y, ld, nb, scal, flag_w, tile_done, epoch);
        return;                                      // (the tiles are the other workgroups' -- the host launches at least one when there are any)
    }
    if (threadIdx.x >= 256) return;
    while (tk <= n_tiles) {
        chol_trail_tile(chol_lds, (int)tk - 1, A, Uf, Winv, b, y, ld, nb, scal, flag_w, tile_done, epoch);
        __syncthreads();                             // (everybody has read s_tk and is done with the tile's LDS)
        if (threadIdx.x == 0) s_tk = atomicAdd(ticket, 1u) - ticket_base;
        __syncthreads();
        tk = s_tk;
    }
}
}  // namespace ba
}  // namespace qsp
