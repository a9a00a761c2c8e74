// dense_chol.hpp -- the interface of the dense f64 blocked Cholesky solve: constants, operand layout and kernel declarations.
// The definitions are in dense_chol_kernels.hpp, which ba_solver.hip alone includes; every other translation unit launches the
// kernels through the declarations below (the object that defines them registers them with the runtime).
//
// The kernels factorise A = L L^T by 64-wide block steps and carry the right-hand side along, y = L^-1 b.  nb = ld / NB.
//   A      row-major, pitch ld, ld a multiple of NB; tiles (i, j) with i <= j are read, and CONSUMED (so is b, from step 0 on)
//   Winv   block k at Winv + k NB NB: W_k^T, W_k = L_kk^-1, element (m, q) of the transpose at [m NB + q]
//   Uf     the factor's block U_kj = W_k A_kj (k < j) TRANSPOSED: element (m, c) at Uf[(j NB + c) ld + k NB + m]
//   y      y[k NB + m], complete for block k once step k - 1 has run
//   scal   doubles: scal[3] is set to 1.0 when a pivot is not positive, scal[5] when a wait of k_chol_solve has run out (never
//          cleared here: the caller does that, and on either must not use the results)
// The backward substitution x_k = W_k^T (y_k - sum_{j > k} U_kj x_j) is the caller's (k_chol_back, eg::k_eg_back).
#pragma once
#include <hip/hip_runtime.h>

namespace qsp {
namespace ba {

constexpr int NB = 64;   // Cholesky block
constexpr int CHOL_THREADS = 320;           // four waves of 4x4 tiles + the panel wave of factor_tile64
constexpr int CHOL_ROWBUF = 4 * 8 * NB;     // factor_tile64: published rows (rb) and rows handed to the panel wave (nx), double-buffered
constexpr int CHOL_LDS_DOUBLES = 3 * NB * NB + CHOL_ROWBUF + NB;
constexpr int CHAIN_LDS_DOUBLES = NB * (NB + 1) + 2 * NB * NB + CHOL_ROWBUF + 3 * NB + 2;
constexpr int TRAIL_LDS_DOUBLES = 3 * NB * NB + NB;
constexpr int CHOL_SOLVE_LDS_DOUBLES = CHAIN_LDS_DOUBLES > TRAIL_LDS_DOUBLES ? CHAIN_LDS_DOUBLES : TRAIL_LDS_DOUBLES;

// One launch per block step, CHOL_THREADS threads and CHOL_LDS_DOUBLES doubles of dynamic LDS each (above the default limit:
// hipFuncAttributeMaxDynamicSharedMemorySize).  k_chol_first, one workgroup: W_0 and y_0.  k_chol_step, k = 0 .. nb - 2 in
// stream order, grid (nb - k - 1, nb - k - 1): block row k of Uf, the trailing update, W_{k+1} and y_{k+1}.
__global__ __launch_bounds__(CHOL_THREADS) void k_chol_first(const double* A, double* Winv, const double* b, double* y, int ld,
                                                             double* scal);
__global__ __launch_bounds__(CHOL_THREADS) void k_chol_step(double* A, double* Uf, double* Winv, double* b, double* y, int ld, int k,
                                                            double* scal);
// The same factorisation, bit for bit, in ONE launch (nb >= 2): 1 + min(n_tiles, compute units - 1) workgroups, CHOL_THREADS threads,
// CHOL_SOLVE_LDS_DOUBLES doubles of LDS.  flag_w [nb] and tile_done [nb nb] hold epochs (zeroed once, epoch != 0 and new for
// every solve); *ticket is a counter that is never reset and ticket_base its value before the launch; n_tiles = nb (nb - 1) / 2
// from nb = 3 on, 0 at nb = 2 (the chain workgroup needs no help there).
__global__ __launch_bounds__(CHOL_THREADS) void k_chol_solve(double* A, double* Uf, double* Winv, double* b, double* y, int ld, int nb, double* scal,
                                                             unsigned* flag_w, unsigned* tile_done, unsigned epoch, unsigned* ticket,
                                                             unsigned ticket_base, unsigned n_tiles);

}  // namespace ba
}  // namespace qsp
