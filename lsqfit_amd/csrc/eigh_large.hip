// Batched symmetric eigensolver for the covariance blocks the svdcut floor binds, 256 < B <= 8192: where the
// one-workgroup solver of eigh_blocks.hip ends (a chain of barrier steps with no arithmetic to speak of), the O(B^3)
// work goes to the matrix pipe.
//
// Two-sided block Jacobi.  Per matrix: A (symmetric, overwritten) and V (= I at the start), row-major in HBM, both
// padded to Bp = B rounded up to the column-block width b = 32.  A sweep is the round-robin tournament of
// eigh_blocks.hip over the nblk = Bp / 32 column blocks: n - 1 steps (n = nblk rounded up to even) of nblk / 2
// disjoint pairs (I, J); with an odd nblk the phantom's partner rests.  A step is five launches, each over all
// matrices and all pairs:
//
//   gather   P = [A_II A_IJ; A_JI A_JJ]                      64 x 64 per pair, contiguous
//   solve    launch_eigh_twosided on the batch of P          P <- Q, orthonormal eigenvectors (two-sided Jacobi in LDS)
//   polish   Q <- Q (3 I - Q^T Q) / 2                        polish_kernel (see below)
//   columns  X[:, I u J] <- X[:, I u J] Q   for X = A and V  rotate_kernel<false>
//   rows     A[I u J, :] <- Q^T A[I u J, :]                  rotate_kernel<true>
//
// so that afterwards the pair's pivot is diagonal.  Pairs of one step touch disjoint columns, then disjoint rows: no
// workgroup waits for another, the kernel boundary publishes each phase.
//
// rotate_kernel: one workgroup = a 64 x 64 tile (64 rows x the pair's two 32-column strips, or the two 32-row strips
// x 64 columns), 4 waves in 2 x 2, each 32 x 32 of the output = 2 x 2 v_mfma_f64_16x16x4_f64 accumulators over the
// 64-deep contraction.  Q and the tile are staged WHOLE in LDS (75 / 80 KB) before the first product, so the update is in
// place.  Both operands are then read with lane-constant bases and compile-time offsets -- the stage loop holds
// ds_read_b64 and MFMAs only (fp64 VALU work is not hidden behind fp64 MFMAs):
//   columns  O[t][c] = sum_k T[t][k] Q[k][c]     A operand lane l = T[l & 15][k0 + (l >> 4)]   (row stride 68: 4 m + k
//                                                distinct over 8 rows), B operand = Q[k0 + (l >> 4)][l & 15] (stride 80)
//   rows     O[k'][t] = sum_k Q[k][k'] T[k][t]   A operand lane l = Q[k0 + (l >> 4)][l & 15], B operand = T likewise
//
// Ragged B: the padding rows and columns of A hold zeros off the diagonal and -1 on it, those of V the unit matrix.
// A rotation between columns that are both exactly zero in a row keeps that row zero, and the inner solver never
// rotates a pair whose off-diagonal entry is exactly zero (its test is |a_pq| > eps |P|_F / 64): the padding stays
// EXACTLY decoupled -- Q holds the unit vectors of the padding indices bit for bit, wherever the ascending order of
// Q's columns moves them.  At the end a column j is a padding column iff V[k][j] == 1 for a padding row k; those are
// left out of the sort.  |A|_F excludes them (each contributes exactly 1 to the sum of squares).
//
// The inner solve is launch_eigh_twosided (eigh_twosided.hip): classical two-sided Jacobi on the pivot itself, in LDS.  The
// pivots of a singular covariance are indefinite as soon as its null space has gathered into whole column blocks (a
// null-null pivot is rounding noise of either sign); to that solver they are ordinary input, and the pivot goes to it as
// it is gathered, with one addition: a floor on its rotation test from the norm of the whole matrix (kPivotFloor).  Until
// then the inner solve was the one-sided solver of eigh_blocks.hip, which diagonalises P^2 and cannot separate eigenvalues
// +l and -l' that agree in magnitude; it needed a diagonal shift of the pivot and still handed back singular blocks from
// 1024 rows on (profiles/eigh_large.txt).  That arithmetic stays reachable for measurements: LSQAMD_EIGH_LARGE_INNER=onesided
// (read per call) gathers with the shift sigma = kShiftOneSided B eps |A|_F and solves with launch_eigh_blocks.
// profiles/eigh_pivots.txt holds the two side by side.
//
// A matrix that has met the stopping test is frozen (the done words go to the device after the sweep): rotate_kernel leaves
// it alone and polish_kernel no longer collects status words for it, so what the caller gets does not depend on how long the
// other matrices of the batch go on.
//
// Convergence: after every sweep off(A)_F^2 and |A|_F^2 per matrix (two launches, fixed summation order) go to one
// pinned record the host reads once per sweep; a matrix is done when off(A)_F <= kOffTol B eps |A|_F (see kOffTol),
// at the latest after kMaxSweeps sweeps.  status 1 (the caller's host route takes the block): not done by then, one of
// its inner solves came back with status 1 (polish_kernel collects the words), or an eigenvalue is not finite.
//
// Between solve and columns one more launch, polish_kernel, makes Q orthonormal to rounding (one Newton-Schulz step on
// MFMA): measured without it (one-sided inner solver), the 64 eps the inner solver's Q is off by add up over the (nblk - 1) x
// sweeps similarities to 7-14 B eps lam_max in the eigenvalues; with it every defect is at most 0.44 of max(B eps lam_max,
// LAPACK's own defect), with either inner solver.  The two-sided solver's rotations accumulate in V the same way; whether its
// defects would hold without the polish has not been measured, so the polish stays.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"

namespace lsqamd_host {   // pool.hip: recycled pinned blocks
void *pinned_take(size_t bytes, size_t *granted);
void pinned_give(void *p, size_t granted, int dev);
}  // namespace lsqamd_host

namespace lsqamd {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kMaxSweeps = 30;
constexpr double kEps = 2.220446049250313e-16;
// Stopping factor.  The iteration has a fixed point: the inner solver leaves a pair alone below its thresholds.  Measured with
// the one-sided inner solver (profiles/eigh_large.txt) off(A)_F then sat at 0.17-0.28 B eps |A|_F for the test matrices of
// 257..513 rows, bit for bit from sweep to sweep; a factor below that level would never be met, 1 was met one or two sweeps
// before the fixed point.  With the two-sided inner solver the sweep that meets 1 ends at about 0.01 for singular blocks of
// 320..2048 rows (profiles/eigh_pivots.txt 3) and every defect of the tests stays below 0.44 of their unit, so the factor stays.
constexpr double kOffTol = 1.0;
// The inner solver leaves a pair alone at or below kPivotFloor eps |A|_F, |A|_F of the WHOLE matrix (gather_kernel writes
// the level per pivot), besides its own test against the pivot's norm.  Without it a null-null pivot of a singular block
// -- rounding noise and nothing else, so its own norm is no scale -- is diagonalised by rotations of arbitrary angle, which
// (as we read it) carry the range-null coupling that the sweep has not reached yet back into the blocks it has already
// cleared.  What is measured (profiles/eigh_pivots.txt 3): without the floor the tail is linear, a factor 5.5 / 1.9 / 1.5
// per sweep at 320 / 1024 / 2048 rows (13 / 26 / more than 30 sweeps); with the floor 9 / 11 / 13 sweeps.  1 / 32:
// everything the floor ever skips sums to off(A)_F <= Bp eps |A|_F / 32, a 32nd of the stopping level; a floor of 1 was
// measured too and saves one more sweep, with nothing left between it and kOffTol.
constexpr double kPivotFloor = 1.0 / 32.0;
// LSQAMD_EIGH_LARGE_INNER=onesided only: the pivot shift in units of B eps |A|_F that the one-sided inner solver needs (see
// the header; 64 left no indefinite pivot up to 513 rows, profiles/eigh_large.txt).
constexpr double kShiftOneSided = 64.0;
constexpr int kBlk = 32, kPiv = 64;
constexpr int LDQ = 80;                       // Q in LDS: rows 16 doubles apart mod 32 banks (4 k-rows x 16 columns per read)
constexpr int LDT_COL = 68, LDT_ROW = 80;     // the tile: read by rows of 4 k (columns role) or like Q (rows role)

constexpr size_t kLdsCol = sizeof(double) * kPiv * (LDQ + LDT_COL), kLdsRow = sizeof(double) * kPiv * (LDQ + LDT_ROW);

constexpr int64_t rup(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// pair `slot` of step s of the round-robin over n (even) players: index n - 1 stays, the others walk round the table
__device__ __forceinline__ void pair_of(int n, int s, int slot, int &p, int &q) {
  const int ia = slot == 0 ? n - 1 : (s + slot) % (n - 1);
  const int ib = slot == 0 ? s : (s - slot + (n - 1)) % (n - 1);
  p = ia < ib ? ia : ib;
  q = ia < ib ? ib : ia;
}

struct Large {
  double *A, *V, *piv;
  int64_t lda, strideA, strideV;   // V: leading dimension Bp
  int32_t B, Bp, nblk, n, npairs, slot0;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// padding of A (zeros, -1 on the diagonal), V = I, no inner solve has failed yet; grid (Bp, nb)
__global__ __launch_bounds__(256) void pad_init_kernel(Large g, int32_t *ibad, int32_t *done) {
  const int64_t i = blockIdx.x, b = blockIdx.y;
  if (i == 0 && threadIdx.x == 0) ibad[b] = done[b] = 0;
  double *a = g.A + b * g.strideA + i * g.lda, *v = g.V + b * g.strideV + i * g.Bp;
  for (int64_t j = threadIdx.x; j < g.Bp; j += 256) {
    if (i >= g.B || j >= g.B) a[j] = i == j ? -1.0 : 0.0;
    v[j] = i == j ? 1.0 : 0.0;
  }
}

// grid (npairs, nb): the pair's pivot, 64 x 64 contiguous, as it is, and floor[pivot] = level * |A_b|_F for the inner
// solver's rotation test (rec: offnorm_kernel's record, npad: the padding's share of it).  SHIFT (the one-sided inner solver
// only): no floor, level * |A_b|_F goes on the pivot's diagonal instead
template <bool SHIFT>
__global__ __launch_bounds__(256) void gather_kernel(Large g, int s, const double *rec, double level, double npad,
                                                     double *floor) {
  const int64_t b = blockIdx.y;
  const double sigma = level * sqrt(rec[2 * b] + rec[2 * b + 1] - npad);
  if (!SHIFT && threadIdx.x == 0) floor[b * g.npairs + blockIdx.x] = sigma;
  int p, q;
  pair_of(g.n, s, (int)blockIdx.x + g.slot0, p, q);
  const double *a = g.A + b * g.strideA;
  double *out = g.piv + (b * g.npairs + blockIdx.x) * (kPiv * kPiv);
  const int c = threadIdx.x & 63;
  const int64_t col = c < kBlk ? p * kBlk + c : q * kBlk + c - kBlk;
  for (int r = threadIdx.x >> 6; r < kPiv; r += 4) {
    const int64_t row = r < kBlk ? p * kBlk + r : q * kBlk + r - kBlk;
    const double v = a[row * g.lda + col];
    out[r * kPiv + c] = SHIFT && r == c ? v + sigma : v;
  }
}

// a wave's 32 x 32 of a 64-deep product from LDS: acc[i][j] += sum_k A[16 i ..][k] B[k][16 j ..], the operands at lane-constant
// bases (A lane l = A[l & 15][l >> 4], B lane l = B[l >> 4][l & 15]) plus compile-time offsets
template <int A_M, int A_K, int B_K>
__device__ __forceinline__ void contract64(const double *abase, const double *bbase, v4d (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < kPiv / 4; ++kk) {
    const double a0 = abase[kk * A_K], a1 = abase[kk * A_K + A_M];
    const double b0 = bbase[kk * B_K], b1 = bbase[kk * B_K + 16];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// Q <- Q (3 I - Q^T Q) / 2, one Newton-Schulz step per pivot: the inner solver's Q is orthonormal to ~ 64 eps (its rotations
// accumulate), and a similarity with such a Q moves the eigenvalues by as much -- once per step, (nblk - 1) x sweeps times.
// The step squares the defect, so what is left is the rounding of this product.  A padding index keeps its unit vector bit
// for bit: its row and column of Q^T Q are those of I, and products with exact zeros are exact.  Also: an inner solve that
// came back with status 1 marks its matrix (ibad; every writer stores the same value).  grid nb * npairs
__global__ __launch_bounds__(256) void polish_kernel(double *piv, const int32_t *istatus, const int32_t *done, int32_t *ibad,
                                                     int32_t npairs) {
  extern __shared__ double lds[];
  double *Qs = lds, *Ms = lds + kPiv * LDQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *Q = piv + (int64_t)blockIdx.x * (kPiv * kPiv);
  if (done[blockIdx.x / npairs] != 0) return;          // the matrix is through: rotate_kernel leaves it alone too
  if (tid == 0 && istatus[blockIdx.x] != 0) ibad[blockIdx.x / npairs] = 1;
  for (int r = wave; r < kPiv; r += 4) Qs[r * LDQ + lane] = Q[r * kPiv + lane];
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1, lm = lane & 15, lk = lane >> 4;
  v4d acc[2][2] = {};
  contract64<16, 4 * LDQ, 4 * LDQ>(Qs + lk * LDQ + wm * 32 + lm, Qs + lk * LDQ + wn * 32 + lm, acc);   // S = Q^T Q
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * 32 + i * 16 + lk + 4 * r, n = wn * 32 + j * 16 + lm;
        Ms[m * LDQ + n] = (m == n ? 1.5 : 0.0) - 0.5 * acc[i][j][r];
        acc[i][j][r] = 0.0;
      }
  __syncthreads();
  contract64<16 * LDQ, 4, 4 * LDQ>(Qs + (wm * 32 + lm) * LDQ + lk, Ms + lk * LDQ + wn * 32 + lm, acc);   // Q M
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * 32 + i * 16 + lk + 4 * r, n = wn * 32 + j * 16 + lm;
        Q[m * kPiv + n] = acc[i][j][r];
      }
}

// ROW = false: X[row0 .. row0 + 64, I u J] <- (same) Q for X = A (blockIdx.z even) and X = V (odd); grid (Bp / 64 up, npairs, 2 nb)
// ROW = true:  A[I u J, col0 .. col0 + 64] <- Q^T (same);                                           grid (Bp / 64 up, npairs, nb)
// A matrix whose done word is set (it met the stopping test in an earlier sweep) is left as it is.
template <bool ROW>
__global__ __launch_bounds__(256) void rotate_kernel(Large g, int s, const int32_t *done) {
  constexpr int LDT = ROW ? LDT_ROW : LDT_COL;
  extern __shared__ double lds[];
  double *Qs = lds, *Ts = lds + kPiv * LDQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = ROW ? blockIdx.z : blockIdx.z >> 1;
  const bool isV = !ROW && (blockIdx.z & 1);
  if (done[b] != 0) return;
  int p, q;
  pair_of(g.n, s, (int)blockIdx.y + g.slot0, p, q);
  const double *Q = g.piv + (b * g.npairs + blockIdx.y) * (kPiv * kPiv);
  double *X = isV ? g.V + b * g.strideV : g.A + b * g.strideA;
  const int64_t ld = isV ? g.Bp : g.lda;
  const int64_t t0 = (int64_t)blockIdx.x * 64;          // first row (columns role) / first column (rows role) of the tile
  // stage Q and the whole tile; lanes run along the contiguous direction of X
  {
    const int c = lane;
    const int64_t strip = c < kBlk ? p * kBlk + c : q * kBlk + c - kBlk;   // columns role: this lane's column of X
    for (int r = wave; r < kPiv; r += 4) {
      Qs[r * LDQ + c] = Q[r * kPiv + c];
      if (ROW) {
        const int64_t row = r < kBlk ? p * kBlk + r : q * kBlk + r - kBlk;
        Ts[r * LDT + c] = t0 + c < g.Bp ? X[row * ld + t0 + c] : 0.0;
      } else {
        Ts[r * LDT + c] = t0 + r < g.Bp ? X[(t0 + r) * ld + strip] : 0.0;
      }
    }
  }
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1, lm = lane & 15, lk = lane >> 4;
  // operand bases: everything that depends on the lane or the wave; the loop below adds compile-time offsets only
  const double *abase = ROW ? Qs + lk * LDQ + wm * 32 + lm : Ts + (wm * 32 + lm) * LDT + lk;
  const double *bbase = ROW ? Ts + lk * LDT + wn * 32 + lm : Qs + lk * LDQ + wn * 32 + lm;
  v4d acc[2][2] = {};
  // A operand: next 16 rows of the output, next 4 k; B operand: next 4 k
  contract64<(ROW ? 16 : 16 * LDT), (ROW ? 4 * LDQ : 4), (ROW ? 4 * LDT : 4 * LDQ)>(abase, bbase, acc);
  // accumulator lane l, register r = O[(l >> 4) + 4 r][l & 15]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * 32 + i * 16 + lk + 4 * r, n = wn * 32 + j * 16 + lm;
        if (ROW) {
          const int64_t row = m < kBlk ? p * kBlk + m : q * kBlk + m - kBlk;
          if (t0 + n < g.Bp) X[row * ld + t0 + n] = acc[i][j][r];
        } else {
          const int64_t col = n < kBlk ? p * kBlk + n : q * kBlk + n - kBlk;
          if (t0 + m < g.Bp) X[(t0 + m) * ld + col] = acc[i][j][r];
        }
      }
}

// rowsq[b][i] = sum_j A_ij^2, rowsq[nb Bp + b Bp + i] = A_ii^2; one wave per row, grid (Bp / 4 up, nb)
__global__ __launch_bounds__(256) void rownorm_kernel(Large g, int32_t nb, double *rowsq) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (i >= g.Bp) return;
  const double *a = g.A + b * g.strideA + i * g.lda;
  double acc = 0.0;
  for (int64_t j = lane; j < g.Bp; j += 64) acc += j == i ? 0.0 : a[j] * a[j];
  acc = wave_sum(acc);
  if (lane == 0) {
    rowsq[b * g.Bp + i] = acc;
    rowsq[((int64_t)nb + b) * g.Bp + i] = a[i] * a[i];
  }
}

// rec[2 b] = off(A_b)_F^2, rec[2 b + 1] = sum of the squared diagonal (padding included); grid nb
__global__ __launch_bounds__(256) void offnorm_kernel(Large g, int32_t nb, const double *rowsq, double *rec) {
  __shared__ double sh[8];
  const int64_t b = blockIdx.x;
  double off = 0.0, dg = 0.0;
  for (int64_t i = threadIdx.x; i < g.Bp; i += 256) {
    off += rowsq[b * g.Bp + i];
    dg += rowsq[((int64_t)nb + b) * g.Bp + i];
  }
  off = wave_sum(off);
  dg = wave_sum(dg);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = off;
    sh[4 + (threadIdx.x >> 6)] = dg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rec[2 * b] = sh[0] + sh[1] + sh[2] + sh[3];
    rec[2 * b + 1] = sh[4] + sh[5] + sh[6] + sh[7];
  }
}

// key[b][j] = A_jj, +inf for a padding column (V[k][j] == 1 for a padding row k); src[b][j] = 0; grid (Bp / 256 up, nb)
__global__ __launch_bounds__(256) void diag_kernel(Large g, double *key, int32_t *src) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= g.Bp) return;
  const double *v = g.V + b * g.strideV;
  bool pad = false;
  for (int64_t k = g.B; k < g.Bp; ++k) pad = pad || v[k * g.Bp + j] == 1.0;
  key[b * g.Bp + j] = pad ? HUGE_VAL : g.A[b * g.strideA + j * g.lda + j];
  src[b * g.Bp + j] = 0;
}

// ascending order by rank (ties by index): src[b][rank] = column; grid (Bp / 256 up, nb)
__global__ __launch_bounds__(256) void rank_kernel(Large g, const double *key, int32_t *src) {
  __shared__ double ks[256];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const double *kb = key + b * g.Bp;
  const double kj = j < g.Bp ? kb[j] : 0.0;
  int rank = 0;
  for (int64_t k0 = 0; k0 < g.Bp; k0 += 256) {
    __syncthreads();
    ks[threadIdx.x] = k0 + threadIdx.x < g.Bp ? kb[k0 + threadIdx.x] : HUGE_VAL;
    __syncthreads();
    const int lim = g.Bp - k0 < 256 ? (int)(g.Bp - k0) : 256;
    for (int k = 0; k < lim; ++k) rank += (ks[k] < kj || (ks[k] == kj && k0 + k < j)) ? 1 : 0;
  }
  if (j < g.Bp) src[b * g.Bp + rank] = (int32_t)j;
}

// A_b[i][r] = V_b[i][src[r]], lam[b][r] = key[src[r]] for i, r < B; sweeps / status of the matrix; grid (B, nb)
__global__ __launch_bounds__(256) void scatter_kernel(Large g, const double *key, const int32_t *src, const int32_t *done,
                                                      const int32_t *ibad, double *lam, int32_t *sweeps, int32_t *status) {
  __shared__ int bad;
  const int64_t i = blockIdx.x, b = blockIdx.y;
  const int32_t *sb = src + b * g.Bp;
  const double *v = g.V + b * g.strideV + i * g.Bp;
  double *a = g.A + b * g.strideA + i * g.lda;
  for (int64_t r = threadIdx.x; r < g.B; r += 256) a[r] = v[sb[r]];
  if (i != 0) return;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int64_t r = threadIdx.x; r < g.B; r += 256) {
    const double l = key[b * g.Bp + sb[r]];
    lam[b * g.B + r] = l;
    if (!(fabs(l) < 1.0e300)) bad = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sweeps[b] = done[b] > 0 ? done[b] : kMaxSweeps;
    status[b] = done[b] > 0 && !bad && !ibad[b] ? 0 : 1;
  }
}

struct Scratch {
  double *V, *piv, *ilam, *rowsq, *rec, *key, *floor;
  int32_t *src, *isweeps, *istatus, *done, *ibad;
  size_t doubles;
};

Scratch carve(int64_t B, int64_t nb, double *base) {
  const int64_t Bp = rup(B, kBlk), npairs = Bp / kBlk / 2;
  Scratch s;
  size_t off = 0;
  auto take = [&](size_t n) {
    double *q = base ? base + off : nullptr;
    off += (size_t)rup((int64_t)n, 32);
    return q;
  };
  s.V = take((size_t)(nb * Bp * Bp));                       // first: the caller may reuse it once the solver is through
  s.piv = take((size_t)(nb * npairs * kPiv * kPiv));        // pivots, overwritten with their eigenvectors Q
  s.ilam = take((size_t)(nb * npairs * kPiv));
  s.rowsq = take((size_t)(2 * nb * Bp));
  s.rec = take((size_t)(2 * nb));
  s.key = take((size_t)(nb * Bp));
  s.src = (int32_t *)take((size_t)(nb * Bp + 1) / 2);
  s.isweeps = (int32_t *)take((size_t)(nb * npairs + 1) / 2);
  s.istatus = (int32_t *)take((size_t)(nb * npairs + 1) / 2);
  s.done = (int32_t *)take((size_t)(nb + 1) / 2);
  s.ibad = (int32_t *)take((size_t)(nb + 1) / 2);
  s.floor = take((size_t)(nb * npairs));                    // per pivot: the floor of the inner solver's rotation test
  s.doubles = off;
  return s;
}

}  // namespace

size_t eigh_large_scratch_doubles(int64_t B, int32_t nb) { return carve(B, nb, nullptr).doubles; }

#define ECHK(expr)                       \
  do {                                   \
    const hipError_t e_ = (expr);        \
    if (e_ != hipSuccess) {              \
      (void)hipStreamSynchronize(st);    /* copies from or to the pinned record may be in flight */ \
      lsqamd_host::pinned_give(pin, granted, -1); \
      return e_;                         \
    }                                    \
  } while (0)

hipError_t launch_eigh_large(hipStream_t st, double *A, int64_t B, int64_t lda, int64_t strideA, int32_t nb, double *scratch,
                             double *lam, int32_t *sweeps, int32_t *status) {
  const int64_t Bp = rup(B, kBlk);
  if (B <= kEighBlocksMax || B > kEighLargeMax || nb < 1 || lda < Bp || strideA < Bp * lda || !scratch || nb > kEighLargeBatchMax)
    return hipErrorInvalidValue;
  const Scratch sc = carve(B, nb, scratch);
  Large g;
  g.A = A; g.V = sc.V; g.piv = sc.piv;
  g.lda = lda; g.strideA = strideA; g.strideV = Bp * Bp;
  g.B = (int32_t)B; g.Bp = (int32_t)Bp;
  g.nblk = (int32_t)(Bp / kBlk);
  g.n = g.nblk + (g.nblk & 1);
  g.npairs = g.nblk / 2;
  g.slot0 = g.nblk & 1;             // odd block count: slot 0 is the phantom's pair, which rests
  const unsigned tiles = (unsigned)((Bp + 63) / 64), unb = (unsigned)nb;
  size_t granted = 0;
  // host record: [2 nb] doubles (off^2, diag^2) read back per sweep, then [nb] int32 (sweep a matrix was done at) sent down
  const size_t rec_bytes = sizeof(double) * 2 * (size_t)nb;
  void *pin = lsqamd_host::pinned_take(rec_bytes + sizeof(int32_t) * (size_t)nb, &granted);
  if (!pin) return hipErrorOutOfMemory;
  double *rec = (double *)pin;
  int32_t *done = (int32_t *)((char *)pin + rec_bytes);
  for (int32_t b = 0; b < nb; ++b) done[b] = 0;          // 0: not yet; > 0: the sweep it was done at; -1: not finite
  {
    static PerDeviceOnce lds_set;   // 75 / 80 KB of dynamic LDS: above the default limit
    ECHK(lds_set.run([] {
      const hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(rotate_kernel<false>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCol);
      const hipError_t e1 = e0 != hipSuccess ? e0 : hipFuncSetAttribute(reinterpret_cast<const void *>(rotate_kernel<true>),
                                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsRow);
      return e1 != hipSuccess ? e1 : hipFuncSetAttribute(reinterpret_cast<const void *>(polish_kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsRow);
    }));
  }
  const double thr = kOffTol * (double)B * kEps, npad = (double)(Bp - B), shift = kShiftOneSided * (double)B * kEps;
  const char *inner = std::getenv("LSQAMD_EIGH_LARGE_INNER");        // read per call; anything but "onesided": the default
  const bool onesided = inner && std::strcmp(inner, "onesided") == 0;
  hipLaunchKernelGGL(pad_init_kernel, dim3((unsigned)Bp, unb), dim3(256), 0, st, g, sc.ibad, sc.done);
  // |A|_F for the inner solver's floor (the pivot shift); every sweep's record replaces it with the same number to rounding
  hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)((Bp + 3) / 4), unb), dim3(256), 0, st, g, nb, sc.rowsq);
  hipLaunchKernelGGL(offnorm_kernel, dim3(unb), dim3(256), 0, st, g, nb, sc.rowsq, sc.rec);
  ECHK(hipGetLastError());
  int32_t open = nb;
  for (int sweep = 0; sweep < kMaxSweeps && open > 0; ++sweep) {
    for (int s = 0; s < g.n - 1; ++s) {
      if (onesided) {
        hipLaunchKernelGGL(gather_kernel<true>, dim3((unsigned)g.npairs, unb), dim3(256), 0, st, g, s, sc.rec, shift, npad,
                           sc.floor);
        ECHK(launch_eigh_blocks(st, sc.piv, kPiv, kPiv, kPiv * kPiv, nb * g.npairs, nullptr, sc.ilam, sc.isweeps, sc.istatus));
      } else {
        hipLaunchKernelGGL(gather_kernel<false>, dim3((unsigned)g.npairs, unb), dim3(256), 0, st, g, s, sc.rec,
                           kPivotFloor * kEps, npad, sc.floor);
        ECHK(launch_eigh_twosided(st, sc.piv, kPiv, kPiv, kPiv * kPiv, nb * g.npairs, sc.ilam, sc.isweeps, sc.istatus,
                                  sc.floor));
      }
      hipLaunchKernelGGL(polish_kernel, dim3((unsigned)(nb * g.npairs)), dim3(256), kLdsRow, st, sc.piv, sc.istatus, sc.done,
                         sc.ibad, g.npairs);
      hipLaunchKernelGGL(rotate_kernel<false>, dim3(tiles, (unsigned)g.npairs, 2 * unb), dim3(256), kLdsCol, st, g, s, sc.done);
      hipLaunchKernelGGL(rotate_kernel<true>, dim3(tiles, (unsigned)g.npairs, unb), dim3(256), kLdsRow, st, g, s, sc.done);
      if (sweep == 0 && s == 0) ECHK(hipGetLastError());   // a launch that cannot run (the LDS sizes) shows here, not a sweep on
    }
    hipLaunchKernelGGL(rownorm_kernel, dim3((unsigned)((Bp + 3) / 4), unb), dim3(256), 0, st, g, nb, sc.rowsq);
    hipLaunchKernelGGL(offnorm_kernel, dim3(unb), dim3(256), 0, st, g, nb, sc.rowsq, sc.rec);
    ECHK(hipGetLastError());
    ECHK(hipMemcpyAsync(rec, sc.rec, rec_bytes, hipMemcpyDeviceToHost, st));
    ECHK(hipStreamSynchronize(st));
    for (int32_t b = 0; b < nb; ++b) {
      if (done[b] != 0) continue;
      const double off2 = rec[2 * b], fro2 = off2 + rec[2 * b + 1] - npad;     // (the padding's diagonal: exactly 1 each)
      if (!std::isfinite(off2) || !std::isfinite(fro2)) done[b] = -1;
      else if (off2 <= thr * thr * fro2) done[b] = sweep + 1;
      if (done[b] != 0) --open;
    }
    // the done words freeze a matrix that is through while others of the batch go on (no kernel reads them before this copy)
    if (open > 0 && open < nb) ECHK(hipMemcpyAsync(sc.done, done, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, st));
  }
  ECHK(hipMemcpyAsync(sc.done, done, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, st));
  const unsigned chunks = (unsigned)((Bp + 255) / 256);
  hipLaunchKernelGGL(diag_kernel, dim3(chunks, unb), dim3(256), 0, st, g, sc.key, sc.src);
  hipLaunchKernelGGL(rank_kernel, dim3(chunks, unb), dim3(256), 0, st, g, sc.key, sc.src);
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)B, unb), dim3(256), 0, st, g, sc.key, sc.src, sc.done, sc.ibad, lam,
                     sweeps, status);
  ECHK(hipGetLastError());
  ECHK(hipStreamSynchronize(st));          // the pinned record goes back to the pool: the copy from it has to be through
  lsqamd_host::pinned_give(pin, granted, -1);
  return hipSuccess;
}

}  // namespace lsqamd
