// QR-grade covariance of the batched engine for fits of up to 32 parameters (solver = 'qr', the reference's default,
// src/lsqfit/_gsl.pyx:571,646-647): (J^T J + Lambda)^-1 and log det(J^T J + Lambda) of every fit of a batch from a Householder
// factorisation of its whitened Jacobian stacked on the prior's whitened rows.  gsl_multifit_nlinear_covar factors the
// Jacobian itself, so its error is ~ cond(J) eps where the normal equations (potrf -> trtri -> product, batch.hip) give
// cond(J)^2 eps.  qr.hip is the single-fit counterpart (CholeskyQR on 128-wide tiles with host round trips between the
// passes: sized for thousands of columns); here a fit is 5 ... 32 columns wide and there are hundreds of them, so the whole
// batch is TWO launches with no host round trip, no shift and no re-orthogonalisation.
//
// Design: TSQR.  Only R is ever kept -- the covariance needs R alone, so no reflector is stored or applied a second time.
//
//   wave panel (panel_qr)   Lanes are rows: a wave holds a 64 x PP panel, one row of PP doubles per lane in VGPRs (PP = 8,
//       16 or 32 at compile time, every index static).  Lanes 0 .. P-1 hold the running upper-triangular R, lanes P .. 63
//       take 64 - P fresh rows per pass (zeros past the end).  Householder on column j: sigma^2 over the lanes below j from a
//       wave butterfly, alpha from lane j; a column that is already zero below the diagonal takes tau = 0 and no reflector.
//       The dots v^T a_k of the columns right of j are reduced up to 16 at a time in a TRANSPOSING butterfly: at each of the
//       first log2(M) exchange steps a lane keeps one half of its partial sums and sends the other, so M columns cost
//       M - 1 + (6 - log2 M) double exchanges instead of 6 M; the finished sums are read back as wave-uniform scalars.
//       Then the rank-1 update.  The order of every sum is fixed: two runs give the same bits.
//   b_qr_reduce_kernel, grid (chunks, B), 256 threads   The four waves split the chunk's rows contiguously, each reduces
//       its share to an R; the four R's meet in LDS (33 KB at PP = 32, rows padded by one double against bank conflicts)
//       and are merged pairwise -- two R's are a 2 P <= 64 row panel for the same routine.  The chunk's R goes to scratch.
//       Rows per chunk are a constant (kQrChunkRows): the split depends on (N, P) only, never on B or the device.
//   b_qr_finish_kernel, grid (B), one wave   merges the chunk R's (P rows per pass), appends the prior as P rows --
//       sqrt(prec_j) e_j for diagonal priors, the rows of the upper Cholesky factor of a dense shared Lambda (computed here,
//       lanes as columns; backward stable in Lambda, which is all a prior needs) -- then log det = 2 sum log|R_jj|, R^-1 by
//       back substitution (lane c solves R x = e_c, R in LDS, every lane reading the same address) and cov = R^-1 R^-T with
//       the P (P + 1) / 2 entries dealt over the lanes, each stored to both triangles from one register.
//
// No atomics, no cross-workgroup waits: the launch boundary publishes the chunk R's.
//
// MFMA does not fit: the panel is at most 32 columns wide and the reflectors of a panel are a dependent chain (column j + 1
// is not known before reflector j has been applied), so there is no product with a K dimension to feed the matrix pipe;
// a blocked (WY) form would need the reflectors this kernel never stores.  Householder's error is columnwise, so no column
// equilibration pass is made.  No norm is scaled against overflow: whitened rows would need entries beyond 1e150.
//
// Rank test: |R_jj| <= P eps max_i |R_ii| (or a value that is not finite, or a non-positive pivot of the dense prior) sets
// info[b] = j + 1 and leaves cov and logdet of that fit NaN -- what a failed pivot of the Cholesky route leaves; the other fits
// of the batch are not touched.
#include <cmath>

#include "batch.h"

#ifndef LSQAMDB_QR_CHUNK_ROWS
#error "LSQAMDB_QR_CHUNK_ROWS is set by the build recipe (lsqfit_amd/build.py QR_CHUNK_ROWS)"
#endif

namespace lsqamd {

constexpr int kQrChunkRows = LSQAMDB_QR_CHUNK_ROWS;   // rows of J one workgroup of b_qr_reduce_kernel reduces
static_assert(kQrChunkRows >= 256 && kQrChunkRows % 4 == 0, "four waves share a chunk");

namespace {

__device__ __forceinline__ double qr_bcast(double v, int src) {   // lane src's value as a wave-uniform scalar
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

__device__ __forceinline__ double qr_wave_sum(double v) {   // to every lane, fixed order
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

constexpr int qr_log2(int m) { return m <= 1 ? 0 : 1 + qr_log2(m >> 1); }
constexpr int qr_group(int left) { return left >= 16 ? 16 : left > 8 ? 16 : left > 4 ? 8 : left > 2 ? 4 : left > 1 ? 2 : 1; }

// a_k -= tau v (v^T a_k) for the M columns from K0 (those at or beyond PP do not exist).  Transposing butterfly: after step s
// a lane holds the sums over 2^(s+1) lanes of M >> (s+1) columns -- the upper half of its columns if its bit 32 >> s is set --
// so after log2 M steps w[0] of lane l is column l >> (6 - log2 M), and the remaining steps are an ordinary butterfly.
template <int PP, int K0, int M>
__device__ __forceinline__ void qr_apply_group(double (&a)[PP], double v, double tv, int lane) {
  constexpr int Q = qr_log2(M);
  double w[M];
#pragma unroll
  for (int i = 0; i < M; ++i) w[i] = K0 + i < PP ? v * a[K0 + i < PP ? K0 + i : 0] : 0.0;
#pragma unroll
  for (int s = 0; s < Q; ++s) {
    const int cnt = M >> (s + 1), mask = 32 >> s;
    const bool up = (lane & mask) != 0;
#pragma unroll
    for (int i = 0; i < cnt; ++i) {
      const double lo = w[i], hi = w[i + cnt];
      w[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, mask, 64);
    }
  }
#pragma unroll
  for (int mask = 32 >> Q; mask > 0; mask >>= 1) w[0] += __shfl_xor(w[0], mask, 64);
#pragma unroll
  for (int i = 0; i < M; ++i)
    if (K0 + i < PP) a[K0 + i] = fma(-tv, qr_bcast(w[0], i << (6 - Q)), a[K0 + i]);
}

template <int PP, int K0>
__device__ __forceinline__ void qr_apply_from(double (&a)[PP], double v, double tv, int P, int lane) {
  if constexpr (K0 < PP) {
    if (K0 < P) {   // (wave-uniform: the columns from P on are padding)
      constexpr int M = qr_group(PP - K0);
      qr_apply_group<PP, K0, M>(a, v, tv, lane);
      qr_apply_from<PP, K0 + M>(a, v, tv, P, lane);
    }
  }
}

template <int PP, int J>
__device__ __forceinline__ void qr_reflect_from(double (&a)[PP], int P, int lane) {
  if constexpr (J < PP) {
    if (J < P) {
      const bool below = lane > J;
      const double x = below ? a[J] : 0.0;
      const double s2 = qr_wave_sum(x * x);
      if (s2 != 0.0) {   // (wave-uniform; a NaN goes on and reaches the rank test)
        const double alpha = qr_bcast(a[J], J);
        const double nrm = sqrt(alpha * alpha + s2);
        const double beta = alpha >= 0.0 ? -nrm : nrm;
        const double v = lane == J ? 1.0 : x / (alpha - beta);   // v_J = 1, zero above
        const double tau = (beta - alpha) / beta;
        qr_apply_from<PP, J + 1>(a, v, tau * v, P, lane);
        a[J] = lane == J ? beta : (below ? 0.0 : a[J]);
      }
      qr_reflect_from<PP, J + 1>(a, P, lane);
    }
  }
}

// the 64 x P panel a (row = lane) -> its R in lanes 0 .. P-1 (zero below the diagonal, exactly); lanes P .. 63: zeros
template <int PP>
__device__ __forceinline__ void panel_qr(double (&a)[PP], int P, int lane) {
  qr_reflect_from<PP, 0>(a, P, lane);
}

template <int PP>
__global__ __launch_bounds__(256) void b_qr_reduce_kernel(const double *J, int64_t j_stride, int64_t ld, int64_t N, int P,
                                                          double *scratch, int chunks) {
  constexpr int LR = PP + 1;
  __shared__ double sR[4][PP * LR];
  const int chunk = blockIdx.x, b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t)chunk * kQrChunkRows;
  const int rows = (int)(N - r0 < kQrChunkRows ? N - r0 : kQrChunkRows);
  const int rpw = (rows + 3) / 4, fresh = 64 - P, npass = (rpw + fresh - 1) / fresh;
  const int64_t w0 = r0 + (int64_t)wave * rpw, w1 = w0 + rpw < r0 + rows ? w0 + rpw : r0 + rows;
  const double *Jb = J + (int64_t)b * j_stride;
  double a[PP];
#pragma unroll
  for (int k = 0; k < PP; ++k) a[k] = 0.0;
  for (int it = 0; it < npass + 2; ++it) {
    bool go = true;
    if (it < npass) {   // fresh rows of this wave's share (PP <= ld: whole double2 loads inside the row, padding zeroed after)
      const int64_t row = w0 + (int64_t)it * fresh + (lane - P);
      if (lane >= P) {
        const bool have = row < w1;
        const double2 *src = reinterpret_cast<const double2 *>(Jb + (have ? row : r0) * ld);
#pragma unroll
        for (int k = 0; k < PP; k += 2) {
          const double2 t = have ? src[k / 2] : make_double2(0.0, 0.0);
          a[k] = k < P ? t.x : 0.0;
          a[k + 1] = k + 1 < P ? t.y : 0.0;
        }
      }
    } else {            // the four R's pairwise: (0, 1) and (2, 3), then (0, 2)
      const int level = it - npass;
      if ((level == 0 || wave == 2) && lane < P) {
#pragma unroll
        for (int k = 0; k < PP; ++k) sR[wave][lane * LR + k] = a[k];
      }
      __syncthreads();
      go = level == 0 ? (wave & 1) == 0 : wave == 0;
      const int partner = level == 0 ? (wave | 1) : 2;
      if (go && lane >= P) {
        const bool have = lane < 2 * P;
#pragma unroll
        for (int k = 0; k < PP; ++k) a[k] = have ? sR[partner][(lane - P) * LR + k] : 0.0;
      }
    }
    if (go) panel_qr<PP>(a, P, lane);
  }
  if (wave == 0 && lane < P) {
    double *dst = scratch + ((int64_t)b * chunks + chunk) * P * P + (int64_t)lane * P;
#pragma unroll
    for (int k = 0; k < PP; ++k)
      if (k < P) dst[k] = a[k];
  }
}

// prior: 0 none, 1 prec[b][P] diagonal, 2 prec[P][P] dense and shared
template <int PP>
__global__ __launch_bounds__(64) void b_qr_finish_kernel(const double *scratch, int chunks, int P, const double *prec, int prior,
                                                         double *cov, int64_t cov_stride, int64_t ldc, double *logdet,
                                                         int32_t *info) {
  constexpr int LR = PP + 1;
  __shared__ double sR[PP * LR], sX[PP * LR];
  const int b = blockIdx.x, lane = threadIdx.x;
  int bad = 0;
  if (prior == 2) {   // Lambda = U^T U, lane c holds column c; row i of U is finished at step i
    double u[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) u[k] = (k < P && lane < P) ? prec[(int64_t)k * P + lane] : 0.0;
#pragma unroll
    for (int i = 0; i < PP; ++i) {
      if (i < P) {
        const double d = qr_bcast(u[i], i);
        if (bad == 0 && !(d > 0.0 && d - d == 0.0)) bad = i + 1;
        const double r = sqrt(d);
        u[i] = lane >= i ? u[i] / r : 0.0;
#pragma unroll
        for (int k = i + 1; k < PP; ++k)
          if (k < P) u[k] = fma(-qr_bcast(u[i], k), u[i], u[k]);
      }
    }
    if (lane < P) {
#pragma unroll
      for (int i = 0; i < PP; ++i) sX[i * LR + lane] = u[i];
    }
    __syncthreads();
  }
  double a[PP];
#pragma unroll
  for (int k = 0; k < PP; ++k) a[k] = 0.0;
  const int npass = chunks + (prior ? 1 : 0), i = lane - P;
  for (int it = 0; it < npass; ++it) {
    if (lane >= P) {
      const bool have = lane < 2 * P;
      if (it < chunks) {
        const double *src = scratch + ((int64_t)b * chunks + it) * P * P + (int64_t)(have ? i : 0) * P;
#pragma unroll
        for (int k = 0; k < PP; ++k) a[k] = (have && k < P) ? src[k < P ? k : 0] : 0.0;
      } else if (prior == 2) {
#pragma unroll
        for (int k = 0; k < PP; ++k) a[k] = (have && k < P) ? sX[i * LR + k] : 0.0;   // (columns from P on were never written)
      } else {
        const double s = have ? sqrt(prec[(int64_t)b * P + i]) : 0.0;
#pragma unroll
        for (int k = 0; k < PP; ++k) a[k] = k == i ? s : 0.0;
      }
    }
    panel_qr<PP>(a, P, lane);
  }
  __syncthreads();   // (sX: the prior's rows have been read)
  // the diagonal: rank test and log det
  double d = 1.0;
#pragma unroll
  for (int k = 0; k < PP; ++k) d = lane == k ? a[k] : d;
  const double ad = lane < P ? fabs(d) : 0.0;
  double big = ad;   // (fmax drops a NaN: the lane that holds one fails the test below)
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) big = fmax(big, __shfl_xor(big, m, 64));
  const bool small = lane < P && !(ad > (double)P * 2.220446049250313e-16 * big && ad - ad == 0.0);
  const unsigned long long fail = __ballot(small);
  if (bad == 0 && fail) bad = __ffsll((long long)fail);
  const double ldet = 2.0 * qr_wave_sum(lane < P ? log(ad) : 0.0);
  const int npk = P * (P + 1) / 2;
  double *C = cov + (int64_t)b * cov_stride;
  if (lane == 0) {
    info[b] = bad;
    logdet[b] = bad ? NAN : ldet;
  }
  if (bad) {   // (wave-uniform)
    for (int e = lane; e < P * P; e += 64) C[(int64_t)(e / P) * ldc + e % P] = NAN;
    return;
  }
  // R to LDS, padded to PP with the unit matrix so that the solve below needs no guards
#pragma unroll
  for (int k = 0; k < PP; ++k)
    if (lane < PP) sR[lane * LR + k] = lane < P ? a[k] : (lane == k ? 1.0 : 0.0);
  __syncthreads();
  // lane c: x = R^-1 e_c by back substitution (x_i = 0 for i > c comes out exactly: their right-hand sides are zero)
  double x[PP];
#pragma unroll
  for (int r = PP - 1; r >= 0; --r) {
    double s = lane == r ? 1.0 : 0.0;
#pragma unroll
    for (int k = r + 1; k < PP; ++k) s = fma(-sR[r * LR + k], x[k], s);
    x[r] = s / sR[r * LR + r];
  }
  if (lane < PP) {
#pragma unroll
    for (int r = 0; r < PP; ++r) sX[r * LR + lane] = x[r];   // sX[r][c] = (R^-1)[r][c], zero below the diagonal
  }
  __syncthreads();
  for (int e = lane; e < npk; e += 64) {   // entry e of the upper triangle, row by row
    int r = 0, rem = e;
    while (rem >= P - r) { rem -= P - r; ++r; }
    const int c = r + rem;
    double s = 0.0;
    for (int k = c; k < P; ++k) s = fma(sX[r * LR + k], sX[c * LR + k], s);
    C[(int64_t)r * ldc + c] = s;
    C[(int64_t)c * ldc + r] = s;
  }
}

}  // namespace

int64_t batch_qr_chunks(int64_t N) { return (N + kQrChunkRows - 1) / kQrChunkRows; }

hipError_t launch_batch_qr(hipStream_t st, const double *J, int64_t j_stride, int64_t ld, int64_t N, int64_t P, int32_t B,
                           const double *prec, int prior, double *scratch, double *cov, int64_t cov_stride, int64_t ldc,
                           double *logdet, int32_t *info) {
  if (P < 1 || P > kBatchQrMaxP || N < 1 || B < 1 || ld < (P <= 8 ? 8 : P <= 16 ? 16 : 32) || (ld & 1)) return hipErrorInvalidValue;
  const int chunks = (int)batch_qr_chunks(N);
  const dim3 grid((unsigned)chunks, (unsigned)B);
  if (P <= 8) {
    hipLaunchKernelGGL(b_qr_reduce_kernel<8>, grid, dim3(256), 0, st, J, j_stride, ld, N, (int)P, scratch, chunks);
    hipLaunchKernelGGL(b_qr_finish_kernel<8>, dim3((unsigned)B), dim3(64), 0, st, scratch, chunks, (int)P, prec, prior, cov,
                       cov_stride, ldc, logdet, info);
  } else if (P <= 16) {
    hipLaunchKernelGGL(b_qr_reduce_kernel<16>, grid, dim3(256), 0, st, J, j_stride, ld, N, (int)P, scratch, chunks);
    hipLaunchKernelGGL(b_qr_finish_kernel<16>, dim3((unsigned)B), dim3(64), 0, st, scratch, chunks, (int)P, prec, prior, cov,
                       cov_stride, ldc, logdet, info);
  } else {
    hipLaunchKernelGGL(b_qr_reduce_kernel<32>, grid, dim3(256), 0, st, J, j_stride, ld, N, (int)P, scratch, chunks);
    hipLaunchKernelGGL(b_qr_finish_kernel<32>, dim3((unsigned)B), dim3(64), 0, st, scratch, chunks, (int)P, prec, prior, cov,
                       cov_stride, ldc, logdet, info);
  }
  return hipGetLastError();
}

}  // namespace lsqamd
