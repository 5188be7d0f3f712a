// Batched symmetric eigensolver for the 64 x 64 pivots of eigh_large.hip (2 <= B <= 64): classical two-sided Jacobi, the
// whole iteration in LDS, ONE workgroup per matrix, grid = n_matrices.
//
// Why not eigh_blocks.hip: that solver is one-sided (it orthogonalises the columns of G = A V, which diagonalises A^2), so
// eigenvalues +l and -l' of an indefinite matrix that agree in magnitude are degenerate there and their eigenvectors stay
// mixed.  The null-null pivots of a singular covariance are rounding noise of either sign: exactly that case.  Here the
// iteration works on A itself, A <- J^T A J, and an indefinite or semidefinite matrix is an ordinary input; there is no
// "no-eigenvector" test.  And a step of that solver is three wave-butterfly dot products per pair; a step here has no
// reduction at all.
//
// Where the data lives: A twice (source and destination of a step, swapped after it) and V, each n x n with row stride
// n + 1 (odd: rows and columns both spread over the banks), n = B rounded up to even; 3 x 64 x 65 x 8 B = 97.5 KB at B = 64.
// The phantom index B of an odd B is a real row and column of exact zeros: it is never rotated (see below), stays zero, and
// is left out of the sort.
//
// A sweep is the round-robin tournament of both other eigensolvers: n - 1 steps of h = n / 2 disjoint pairs (p_k, q_k),
// k = 0 .. h - 1.  The pairs cut A into a grid of 2 x 2 blocks X_kl = A[{p_k, q_k}, {p_l, q_l}], and the whole step is
//
//   X_kl <- J_k^T X_kl J_l            J_k = [c_k s_k; -s_k c_k], the rotation that annihilates the off-diagonal of X_kk
//
// ONE THREAD PER BLOCK k <= l (528 at B = 64: 9 waves).  The thread reads its four entries and the three entries of X_kk
// and of X_ll from the source copy, computes (c, s) of both rotations itself -- every thread that needs J_k computes the
// same bits from the same three numbers, which costs arithmetic and saves the barrier a broadcast would need -- and writes
// X_kl and its transpose to the destination copy: A stays symmetric bit for bit.  Every entry of the destination is
// written in every step (a pair that is left alone has J = I: c = 1, s = 0, products with those are exact), so the copies
// swap roles with ONE barrier per step.
//
// V <- V J in place, with the rotations the thread holds already: J_m is known to the 32 threads (m, l >= m) and
// (k < m, m), i.e. one per "other" index j = 0 .. h - 1; thread j rotates rows j and j + h of the columns (p_m, q_m).  Every
// element of V is touched by one thread per step, and nobody else reads it before the barrier.
//
// Rotations in Rutishauser's form: theta = (a_qq - a_pp) / 2 a_pq, t = sign(theta) / (|theta| + sqrt(1 + theta^2)),
// c = 1 / sqrt(1 + t^2), s = c t; the diagonal block becomes a_pp - t a_pq, a_qq + t a_pq and EXACT zeros off the diagonal.
//
// Which pairs rotate: |a_pq| > eps |A|_F / B, with |A|_F measured once while the matrix is loaded.  Everything that is
// ever skipped sums to off(A)_F <= eps |A|_F, so noise is not chased; the iteration ends with the first sweep without a
// rotation, at the latest after kMaxSweeps (status 1; also when an eigenvalue is not finite -- the test is written so that
// a NaN means "no rotation").  A caller whose matrices are pivots of a larger one can raise the threshold to a level taken
// from that matrix (floor[b], common.h; why: eigh_large.hip, kPivotFloor).
//
// What eigh_large.hip relies on: a row and column that are exactly zero off the diagonal are never rotated (0 > thr is
// false whatever thr), rotations of other pairs combine exact zeros only, so the index stays EXACTLY decoupled and its
// column of V is its unit vector bit for bit, wherever the ascending order moves it.  No diagonal shift, no perturbation.
//
// Measurements: profiles/eigh_pivots.txt.
#include <cmath>

#include "common.h"

namespace lsqamd {
namespace {

constexpr int kMaxSweeps = 30;
constexpr double kEps = 2.220446049250313e-16;
constexpr int kPivMax = 64;
constexpr int kThreadsMax = 576;     // 32 * 33 / 2 = 528 blocks, in whole waves

struct Rot {
  double c, s, t;
  bool on;
};

// the rotation of a pair from its diagonal block.  Every thread that needs it runs these very instructions on the same
// three numbers (no contraction that could differ between the places this is inlined at).
__device__ __forceinline__ Rot rotation(double app, double aqq, double apq, double thr) {
#pragma clang fp contract(off)
  Rot r = {1.0, 0.0, 0.0, false};
  if (!(fabs(apq) > thr)) return r;              // (a NaN: no rotation)
  const double theta = (aqq - app) / (2.0 * apq);
  // (theta^2 overflows for a tiny a_pq; 1 / (2 theta) is the same number to rounding beyond 1e8)
  r.t = fabs(theta) > 1.0e8 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
  r.c = 1.0 / sqrt(1.0 + r.t * r.t);
  r.s = r.c * r.t;
  r.on = true;
  return r;
}

// pair `slot` of step s of the round-robin over n (even) players: index n - 1 stays, the others walk round the table
// (s + slot and s - slot + n - 1 are below 2 (n - 1): no division)
__device__ __forceinline__ void pair_of(int n, int s, int slot, int &p, int &q) {
  int ia = s + slot, ib = s - slot + (n - 1);
  ia = ia >= n - 1 ? ia - (n - 1) : ia;
  ib = ib >= n - 1 ? ib - (n - 1) : ib;
  if (slot == 0) {
    ia = n - 1;
    ib = s;
  }
  p = ia < ib ? ia : ib;
  q = ia < ib ? ib : ia;
}

// rows r0 and r0 + h of V, columns (p, q) <- the same times J
__device__ __forceinline__ void rotate_v(double *V, int ld, int n, int h, int r0, int p, int q, const Rot &j) {
  if (!j.on) return;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int r = r0 + e * h;
    if (r < n) {
      const double vp = V[r * ld + p], vq = V[r * ld + q];
      V[r * ld + p] = j.c * vp - j.s * vq;
      V[r * ld + q] = j.s * vp + j.c * vq;
    }
  }
}

__global__ __launch_bounds__(kThreadsMax) void eigh_twosided_kernel(double *A, int B, int64_t lda, int64_t strideA,
                                                                   double *lam_out, int32_t *sweeps_out, int32_t *status_out,
                                                                   const double *floor) {
  extern __shared__ double lds[];
  __shared__ double lam_s[kPivMax];
  __shared__ int src_s[kPivMax];
  __shared__ double red_s[kThreadsMax / 64];
  __shared__ int rot_cnt[2];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int n = B + (B & 1), h = n >> 1, ld = n + 1;
  double *a = A + (int64_t)blockIdx.x * strideA;
  double *S = lds, *D = lds + n * ld, *V = lds + 2 * n * ld;
  // S = A from its upper triangle (symmetric bit for bit whatever the caller's lower triangle holds), zeros in the phantom's
  // row and column, V = I, |A|_F^2
  double fro2 = 0.0;
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const double v = hi < B ? a[lo * lda + hi] : 0.0;
    S[i * ld + j] = v;
    V[i * ld + j] = i == j ? 1.0 : 0.0;
    fro2 += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fro2 += __shfl_xor(fro2, o, 64);
  if (lane == 0) red_s[wave] = fro2;
  if (tid == 0) rot_cnt[0] = rot_cnt[1] = 0;
  __syncthreads();
  fro2 = 0.0;
  for (int w = 0; w < nw; ++w) fro2 += red_s[w];
  double thr = kEps * sqrt(fro2) / B;
  if (floor) thr = fmax(thr, floor[blockIdx.x]);   // (a NaN floor: fmax keeps the matrix's own threshold)
  // this thread's block (k, l), k <= l, row-major over the upper triangle of the h x h grid; k = h: none
  int k = 0, l = tid;
  while (k < h && l >= h - k) {
    l -= h - k;
    ++k;
  }
  l += k;
  const bool work = k < h;
  volatile int *cnt = rot_cnt;
  int prev[2] = {0, 0};
  int sweeps = 0;
  bool converged = false;
  for (int sweep = 0; sweep < kMaxSweeps && !converged; ++sweep) {
    for (int s = 0; s < n - 1; ++s) {
      if (work) {
        int pk, qk, pl, ql;
        pair_of(n, s, k, pk, qk);
        pair_of(n, s, l, pl, ql);
        const Rot jk = rotation(S[pk * ld + pk], S[qk * ld + qk], S[pk * ld + qk], thr);
        const Rot jl = rotation(S[pl * ld + pl], S[ql * ld + ql], S[pl * ld + ql], thr);
        if (k == l) {
          const double app = S[pk * ld + pk], aqq = S[qk * ld + qk], apq = S[pk * ld + qk];
          D[pk * ld + pk] = jk.on ? app - jk.t * apq : app;
          D[qk * ld + qk] = jk.on ? aqq + jk.t * apq : aqq;
          D[pk * ld + qk] = D[qk * ld + pk] = jk.on ? 0.0 : apq;
          if (jk.on) atomicAdd(&rot_cnt[sweep & 1], 1);
          rotate_v(V, ld, n, h, k, pk, qk, jk);
        } else {
          const double xpp = S[pk * ld + pl], xpq = S[pk * ld + ql], xqp = S[qk * ld + pl], xqq = S[qk * ld + ql];
          // Y = X J_l (columns), X' = J_k^T Y (rows)
          const double ypp = jl.c * xpp - jl.s * xpq, ypq = jl.s * xpp + jl.c * xpq;
          const double yqp = jl.c * xqp - jl.s * xqq, yqq = jl.s * xqp + jl.c * xqq;
          const double zpp = jk.c * ypp - jk.s * yqp, zqp = jk.s * ypp + jk.c * yqp;
          const double zpq = jk.c * ypq - jk.s * yqq, zqq = jk.s * ypq + jk.c * yqq;
          D[pk * ld + pl] = D[pl * ld + pk] = zpp;
          D[pk * ld + ql] = D[ql * ld + pk] = zpq;
          D[qk * ld + pl] = D[pl * ld + qk] = zqp;
          D[qk * ld + ql] = D[ql * ld + qk] = zqq;
          rotate_v(V, ld, n, h, l, pk, qk, jk);
          rotate_v(V, ld, n, h, k, pl, ql, jl);
        }
      }
      __syncthreads();          // the step's one barrier: the destination is complete, the source is free
      double *t = S;
      S = D;
      D = t;
    }
    // rotations of this sweep: counter (sweep & 1) is next written two sweeps on, behind barriers every wave has to pass
    // after this read, so all threads see one value and leave the loop together
    const int now = cnt[sweep & 1];
    sweeps = sweep + 1;
    converged = now == prev[sweep & 1];
    prev[sweep & 1] = now;
  }
  for (int j = tid; j < B; j += nt) {
    lam_s[j] = S[j * ld + j];
    src_s[j] = 0;                // (NaN eigenvalues can share a rank: no slot is left unset)
  }
  __syncthreads();
  // ascending order by rank (ties by index): src_s[rank] = column
  for (int j = tid; j < B; j += nt) {
    const double lj = lam_s[j];
    int rank = 0;
    for (int m = 0; m < B; ++m) {
      const double lm = lam_s[m];
      rank += (lm < lj || (lm == lj && m < j)) ? 1 : 0;
    }
    src_s[rank] = j;
  }
  __syncthreads();
  for (int idx = tid; idx < B * B; idx += nt) {
    const int i = idx / B, r = idx - i * B;
    a[i * lda + r] = V[i * ld + src_s[r]];
  }
  for (int r = tid; r < B; r += nt) lam_out[(int64_t)blockIdx.x * B + r] = lam_s[src_s[r]];
  if (tid == 0) {
    bool finite = fro2 < HUGE_VAL;         // (an infinity or NaN off the diagonal stops every rotation: it shows here only)
    for (int j = 0; j < B; ++j) finite = finite && fabs(lam_s[j]) < 1.0e300;
    sweeps_out[blockIdx.x] = sweeps;
    status_out[blockIdx.x] = converged && finite ? 0 : 1;
  }
}

}  // namespace

hipError_t launch_eigh_twosided(hipStream_t st, double *A, int64_t B, int64_t lda, int64_t strideA, int32_t nb, double *lam,
                                int32_t *sweeps, int32_t *status, const double *floor) {
  if (B < 2 || B > kPivMax || nb < 1 || lda < B || !A || !lam || !sweeps || !status) return hipErrorInvalidValue;
  const int64_t n = B + (B & 1), h = n / 2;
  const size_t lds = sizeof(double) * (size_t)(3 * n * (n + 1));
  static PerDeviceMax lds_set;   // per device, thread-safe (common.h); above the default limit from n = 52 on
  const hipError_t e = lds_set.ensure(lds, [](size_t want) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(eigh_twosided_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)want);
  });
  if (e != hipSuccess) return e;
  const unsigned threads = (unsigned)((h * (h + 1) / 2 + 63) / 64 * 64);
  hipLaunchKernelGGL(eigh_twosided_kernel, dim3((unsigned)nb), dim3(threads), lds, st, A, (int)B, lda, strideA, lam, sweeps,
                     status, floor);
  return hipGetLastError();
}

}  // namespace lsqamd
