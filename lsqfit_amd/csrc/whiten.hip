// Whitening set-up on the device: the O(B^3) part of what nonlinear_fit obtains from
// gvar.PDF(...) at src/lsqfit/__init__.py:1892-1900 (per covariance block: factor the correlation
// matrix, build the weights W with W^T W = inv(C), log det C; svdcut semantics
// doc/source/overview.rst:1546-1606).  gvar eigen-decomposes every block on the host; when the
// svdcut floor touches no mode (the usual case) any W with W^T W = inv(C) gives the same chi2,
// J^T J, J^T f, p, cov and logGBF, so this path uses the Cholesky factor:
//
//   C = D corr D,  corr = U^T U  (potrf_upper, batched over same-size blocks)
//   Wl = U^-T (trtri)            W = Wl D^-1,   stored transposed: Wt = D^-1 U^-1 (upper triangular)
//   log det C = 2 sum log U_jj + 2 sum log sd_j
//   prior blocks also need inv(C) = W^T W (TN SYRK of W, as the post-fit covariance does)
//
// and decides ON THE DEVICE whether the floor could touch a mode: rigorous bounds first
// (lambda_max <= max_i sum_j |corr_ij|, lambda_min >= 1 / |Wl|_F^2 since |inv(corr)|_2 <= tr inv(corr)),
// then -- only for blocks the bounds leave undecided -- inverse iteration with the factor
// (u <- Wl^T Wl u, 40 sweeps).  Blocks whose floor may bind (status 1) or that are not positive
// definite (status 2) take the eigen route, which is what gvar does for every block:
// lsqamd_whiten_blocks_eig below (the batched Jacobi solvers of eigh_blocks.hip, up to 256 rows, and eigh_large.hip, up
// to 8192, + eig_weights_kernel), LAPACK on the host (lsqfit_amd/whiten.py) above that.
#include <cmath>
#include <vector>

#include "common.h"

namespace lsqamd {
namespace {

constexpr int64_t rup(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

__device__ __forceinline__ double wsum_w(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sd[b][i] = sqrt(C_b[i][i]); bad[b] = 1 when a variance is not positive and finite
__global__ __launch_bounds__(256) void sdev_kernel(const double *A, int64_t B, int64_t lda, int64_t strideA,
                                                   double *sd, double *logsd_sum, int32_t *bad) {
  __shared__ double sh[4];
  const double *a = A + (int64_t)blockIdx.x * strideA;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 256) {
    const double v = a[i * lda + i];
    const bool ok = v > 0.0 && v < 1.0e300;
    if (!ok) bad[blockIdx.x] = 1;
    const double s = ok ? sqrt(v) : 1.0;
    sd[(int64_t)blockIdx.x * B + i] = s;
    acc += log(s);
  }
  acc = wsum_w(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) logsd_sum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// A_b <- corr_b = C_b / (sd_i sd_j) in place; rowsum[b][i] = sum_j |corr_ij|  (one wave per row)
__global__ __launch_bounds__(256) void to_corr_kernel(double *A, int64_t B, int64_t lda, int64_t strideA,
                                                      const double *sd, double *rowsum) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  double *a = A + (int64_t)blockIdx.y * strideA + i * lda;
  const double *s = sd + (int64_t)blockIdx.y * B;
  const double si = 1.0 / s[i];
  double acc = 0.0;
  for (int64_t j = lane; j < B; j += 64) {
    const double v = (j == i) ? 1.0 : a[j] * si / s[j];
    a[j] = v;
    acc += fabs(v);
  }
  acc = wsum_w(acc);
  if (lane == 0) rowsum[(int64_t)blockIdx.y * B + i] = acc;
}

// out[b] = sum_j log U_b[j][j]
__global__ __launch_bounds__(256) void logdiag_batched_kernel(const double *A, int64_t B, int64_t lda,
                                                              int64_t strideA, double *out) {
  __shared__ double sh[4];
  const double *a = A + (int64_t)blockIdx.x * strideA;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < B; j += 256) acc += log(a[j * lda + j]);
  acc = wsum_w(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// fro2[b][i] = sum_j Wl_b[i][j]^2 (row i of the lower-triangular inverse factor: j <= i);
// optionally W_b[i][j] = Wl_b[i][j] / sd_j (the untransposed weights, for inv(C) = W^T W)
__global__ __launch_bounds__(256) void inv_rows_kernel(const double *Wl, int64_t B, int64_t ldw, int64_t strideW,
                                                       const double *sd, double *W, double *fro2) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const double *w = Wl + (int64_t)blockIdx.y * strideW + i * ldw;
  double *o = W ? W + (int64_t)blockIdx.y * strideW + i * ldw : nullptr;
  const double *s = sd + (int64_t)blockIdx.y * B;
  double acc = 0.0;
  for (int64_t j = lane; j < B; j += 64) {
    const double v = j <= i ? w[j] : 0.0;
    acc += v * v;
    if (o) o[j] = v / s[j];
  }
  acc = wsum_w(acc);
  if (lane == 0) fro2[(int64_t)blockIdx.y * B + i] = acc;
}

// Wt_b row i: scaled by 1 / sd_i, entries left of the diagonal cleared (Wt = D^-1 U^-1 is upper triangular)
__global__ __launch_bounds__(256) void wt_rows_kernel(double *wt, const double *sd, int64_t B) {
  const int64_t i = blockIdx.x, b = blockIdx.y;
  const double s = 1.0 / sd[b * B + i];
  double *row = wt + (b * B + i) * B;
  for (int64_t j = threadIdx.x; j < B; j += 256) row[j] = j >= i ? row[j] * s : 0.0;
}

// u <- w / |w|, |w|^2 given in *nrm2
__global__ __launch_bounds__(256) void normalise_kernel(const double *w, const double *nrm2, double *u, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) u[i] = w[i] / sqrt(nrm2[0]);
}

struct Plan {
  int64_t ldw, strideA;
  double *A, *Wl, *uinv, *sd, *rowsum, *fro2, *logsd, *logu, *vec, *partial, *scal;
  int32_t *info, *bad;
  size_t bytes, readback;
};

Plan make_plan(int64_t B, int64_t nb, void *base) {
  Plan p;
  p.ldw = rup(B, 16);
  p.strideA = B * p.ldw;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void *q = base ? (char *)base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return q;
  };
  p.A = (double *)take(sizeof(double) * nb * p.strideA);
  p.Wl = (double *)take(sizeof(double) * nb * p.strideA);
  p.uinv = (double *)take(potrf_work_bytes(B) * nb);
  p.sd = (double *)take(sizeof(double) * nb * B);
  // (what the host reads back, in one piece: rowsum .. bad are fetched by ONE copy, see lsqamd_whiten_blocks)
  p.rowsum = (double *)take(sizeof(double) * nb * B);
  p.fro2 = (double *)take(sizeof(double) * nb * B);
  p.logsd = (double *)take(sizeof(double) * nb);
  p.logu = (double *)take(sizeof(double) * nb);
  p.info = (int32_t *)take(sizeof(int32_t) * nb);
  p.bad = (int32_t *)take(sizeof(int32_t) * nb);
  p.readback = (size_t)((char *)p.bad - (char *)p.rowsum) + sizeof(int32_t) * (size_t)nb;
  p.vec = (double *)take(sizeof(double) * 3 * B);
  p.partial = (double *)take(sizeof(double) * (256 * B > 2048 ? 256 * B : 2048));
  p.scal = (double *)take(sizeof(double) * 8);
  p.bytes = off;
  return p;
}

// The weights of the eigen-mode route (doc/source/overview.rst:1546-1606) from (lam ascending, V) of the correlation
// matrix, as lsqfit_amd/whiten.py:_regulate_block makes them; one workgroup per block.  floor = |svdcut| lam_max:
// svdcut > 0 raises the nmod modes below it to the floor, svdcut < 0 drops them (kept columns move to the front, the
// rest of Wt is zero).  Wt[i][k] = V[i][k] / (sd_i sqrt(lamreg_k)), contiguous B x B; W (or null) = Wt transposed
// with leading dimension ldW, for inv(C) = W^T W; vec (or null) = V, contiguous.  status: the solver's on entry;
// on exit 2 when a variance or a kept lamreg is not positive, 1 when the result would hang on rounding (below);
// the weights are then not to be used.
__global__ __launch_bounds__(256) void eig_weights_kernel(const double *V, int64_t B, int64_t ldv, int64_t strideV,
                                                          const double *lam, const double *sd, const double *logsd,
                                                          const int32_t *bad, double svdcut, double *wt, double *W,
                                                          int64_t ldW, int64_t strideW, double *vec, double *logdet,
                                                          int32_t *modes, int32_t *nmod, int32_t *status, double *rs_big) {
  __shared__ double rs_lds[256];  // 1 / sqrt(lamreg_k), 0 for a dropped mode (above 256 rows: rs_big, and eig_spread_kernel makes the weights)
  __shared__ double sh[4];
  __shared__ int n_low, not_pd, fragile;
  const int64_t b = blockIdx.x;
  const int t = threadIdx.x;
  const double *l = lam + b * B, *s = sd + b * B, *v = V + b * strideV;
  double *rs = rs_big ? rs_big + b * B : rs_lds;
  if (t == 0) n_low = not_pd = fragile = 0;
  __syncthreads();
  const double cut = fabs(svdcut), floor = cut * l[B - 1];
  int cnt = 0;
  for (int64_t k = t; k < B; k += 256) cnt += cut != 0.0 && l[k] < floor ? 1 : 0;
  if (cnt) atomicAdd(&n_low, cnt);
  __syncthreads();
  const int nm = n_low, first = svdcut < 0.0 ? nm : 0;   // lam ascends: the low modes are the first nm
  double acc = 0.0;
  for (int64_t k = t; k < B; k += 256) {
    const bool low = cut != 0.0 && l[k] < floor;
    const double lr = low && svdcut > 0.0 ? floor : l[k];
    const bool kept = k >= first;
    if (kept && !(lr > 0.0 && lr < 1.0e300)) not_pd = 1;
    // The solver's eigenvalues are good to ~ B eps lam_max ABSOLUTELY (as LAPACK's are).  Where the result leans on more than
    // that -- a mode kept at its own value so small that its relative error passes 1e-9, or a mode within rounding of the
    // floor, so that nmod hangs on it -- the numbers are rounding-dependent, and the block goes to the host, whose LAPACK
    // route gives the bits the reference's own eigh gives (the printed fits of examples/y-noerr.out ride on them).
    const double unit = (double)B * 2.220446049250313e-16 * l[B - 1];
    if ((kept && !low && lr < 1.0e9 * unit) || (cut != 0.0 && fabs(l[k] - floor) < 16.0 * unit)) fragile = 1;
    rs[k] = kept && lr > 0.0 ? 1.0 / sqrt(lr) : 0.0;
    acc += kept && lr > 0.0 ? log(lr) : 0.0;
  }
  acc = wsum_w(acc);
  if ((t & 63) == 0) sh[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    logdet[b] = sh[0] + sh[1] + sh[2] + sh[3] + 2.0 * logsd[b];
    modes[b] = (int32_t)(B - first);
    nmod[b] = nm;
    if (bad[b] || not_pd) status[b] = 2;
    else if (fragile && status[b] == 0) status[b] = 1;
  }
  if (rs_big) return;
  for (int64_t idx = t; idx < B * B; idx += 256) {
    const int64_t i = idx / B, k = idx - i * B, src = k + first;
    const double w = src < B ? v[i * ldv + src] * rs[src] / s[i] : 0.0;
    wt[b * B * B + idx] = w;
    if (W) W[b * strideW + k * ldW + i] = w;
    if (vec) vec[b * B * B + idx] = v[i * ldv + k];
  }
}

// the weights pass of eig_weights_kernel for blocks above 256 rows: row i of Wt_b, column i of W_b; grid (B, nb)
__global__ __launch_bounds__(256) void eig_spread_kernel(const double *V, int64_t B, int64_t ldv, int64_t strideV,
                                                         const double *sd, const double *rs_big, double svdcut,
                                                         const int32_t *nmod, double *wt, double *W, int64_t ldW,
                                                         int64_t strideW, double *vec) {
  const int64_t i = blockIdx.x, b = blockIdx.y;
  const double *v = V + b * strideV + i * ldv, *rs = rs_big + b * B;
  const int64_t first = svdcut < 0.0 ? nmod[b] : 0;
  const double si = sd[b * B + i];
  for (int64_t k = threadIdx.x; k < B; k += 256) {
    const int64_t src = k + first;
    const double w = src < B ? v[src] * rs[src] / si : 0.0;
    wt[(b * B + i) * B + k] = w;
    if (W) W[b * strideW + k * ldW + i] = w;
    if (vec) vec[(b * B + i) * B + k] = v[k];
  }
}

// dst_b[i][0 .. B) = src_b[i][0 .. B): contiguous B x B blocks -> blocks with leading dimension ldd, strided apart
__global__ __launch_bounds__(256) void spread_rows_kernel(const double *src, int64_t B, double *dst, int64_t ldd,
                                                          int64_t strided) {
  const int64_t i = blockIdx.x, b = blockIdx.y;
  for (int64_t j = threadIdx.x; j < B; j += 256) dst[b * strided + i * ldd + j] = src[(b * B + i) * B + j];
}

struct EigPlan {
  int64_t ldw, strideA, strideS;
  double *A, *slab, *W, *sd, *rowsum, *logsd, *logdet, *rs;
  int32_t *modes, *nmod, *sweeps, *status, *bad;
  size_t bytes, readback;
};

EigPlan make_eig_plan(int64_t B, int64_t nb, void *base) {
  EigPlan p;
  const bool large = B > kEighBlocksMax;   // eigh_large.hip: rows and columns padded to 32, W in the solver's V when it is through
  p.ldw = rup(B, large ? 32 : 16);
  p.strideA = (large ? p.ldw : B) * p.ldw;
  p.strideS = large ? p.ldw * p.ldw : (int64_t)eigh_blocks_slab_doubles(B, p.ldw);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void *q = base ? (char *)base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return q;
  };
  p.A = (double *)take(sizeof(double) * nb * p.strideA);          // covariance -> correlation -> eigenvectors, in place
  // the solver's columns (B > 64) or, above 256 rows, all of eigh_large's scratch; free again behind it
  p.slab = (double *)take(sizeof(double) * (large ? eigh_large_scratch_doubles(B, (int32_t)nb) : (size_t)(nb * p.strideS)));
  p.rs = large ? (double *)take(sizeof(double) * nb * B) : nullptr;   // eig_weights_kernel's 1 / sqrt(lamreg) (in LDS up to 256 rows)
  // W = Wt^T for inv(C): in the slab where there is one, in a buffer of its own for the LDS-resident sizes
  p.W = p.strideS ? p.slab : (double *)take(sizeof(double) * nb * p.strideA);
  p.sd = (double *)take(sizeof(double) * nb * B);
  p.rowsum = (double *)take(sizeof(double) * nb * B);
  p.logsd = (double *)take(sizeof(double) * nb);
  // (what the host reads back, in one piece: logdet .. bad)
  p.logdet = (double *)take(sizeof(double) * nb);
  p.modes = (int32_t *)take(sizeof(int32_t) * nb);
  p.nmod = (int32_t *)take(sizeof(int32_t) * nb);
  p.sweeps = (int32_t *)take(sizeof(int32_t) * nb);
  p.status = (int32_t *)take(sizeof(int32_t) * nb);
  p.bad = (int32_t *)take(sizeof(int32_t) * nb);
  p.readback = (size_t)((char *)p.bad - (char *)p.logdet) + sizeof(int32_t) * (size_t)nb;
  p.bytes = off;
  return p;
}

#define WCHK(expr)                          \
  do {                                      \
    if ((expr) != hipSuccess) return LSQAMD_EHIP; \
  } while (0)

}  // namespace
}  // namespace lsqamd

using namespace lsqamd;

extern "C" {

size_t lsqamd_whiten_work_bytes(int64_t block_size, int32_t n_blocks) try {
  if (block_size < 1 || n_blocks < 1) return 0;
  return make_plan(block_size, n_blocks, nullptr).bytes + 256;
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_whiten_blocks(void *stream, int64_t B, int32_t nb, const double *cov, double svdcut,
                         double *wt_out, double *prec_out, void *dev_work, size_t work_bytes,
                         double *logdet_out, double *lam_min_out, double *lam_max_out, int32_t *status_out) try {
  if (B < 1 || nb < 1 || !cov || !wt_out || !dev_work || !logdet_out || !status_out) return LSQAMD_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char *base = (char *)dev_work;
  const size_t pad = (size_t)((-(intptr_t)base) & 255);
  if (work_bytes < pad) return LSQAMD_ENOMEM;
  Plan p = make_plan(B, nb, base + pad);
  if (work_bytes < p.bytes + pad) return LSQAMD_ENOMEM;
  const int64_t ldw = p.ldw, sA = p.strideA;
  // covariance blocks (host or device memory, contiguous [nb][B][B]) -> A (ldw)
  WCHK(hipMemcpy2DAsync(p.A, sizeof(double) * ldw, cov, sizeof(double) * B, sizeof(double) * B, (size_t)(nb * B),
                        hipMemcpyDefault, st));
  WCHK(hipMemsetAsync(p.bad, 0, sizeof(int32_t) * nb, st));
  hipLaunchKernelGGL(sdev_kernel, dim3((unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA, p.sd, p.logsd, p.bad);
  hipLaunchKernelGGL(to_corr_kernel, dim3((unsigned)((B + 3) / 4), (unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA,
                     p.sd, p.rowsum);
  const int64_t sW = (int64_t)(potrf_work_bytes(B) / sizeof(double));
  WCHK(potrf_upper_batched(st, p.A, B, ldw, B, p.uinv, p.info, nb, sA, sW, nullptr));
  hipLaunchKernelGGL(logdiag_batched_kernel, dim3((unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA, p.logu);
  WCHK(trtri_upper_to_lower_T_batched(st, p.A, B, ldw, p.uinv, p.Wl, ldw, nb, sA, sW, sA));
  // A is free from here on: it takes W = Wl D^-1 when inv(C) is wanted
  hipLaunchKernelGGL(inv_rows_kernel, dim3((unsigned)((B + 3) / 4), (unsigned)nb), dim3(256), 0, st, p.Wl, B, ldw, sA,
                     p.sd, prec_out ? p.A : nullptr, p.fro2);
  // Wt_b[i][j] = Wl_b[j][i] / sd_i : transposed weights, contiguous B x B as lsqamd_set_data takes them
  WCHK(launch_transpose_scale(st, p.Wl, ldw, wt_out, B, B, B, nullptr, nullptr, nb, sA, B * B));
  hipLaunchKernelGGL(wt_rows_kernel, dim3((unsigned)B, (unsigned)nb), dim3(256), 0, st, wt_out, p.sd, B);
  if (prec_out) {
    GemmTN g;   // inv(C_b) = W_b^T W_b (upper tiles), then mirrored
    g.X = p.A; g.Y = p.A; g.ldx = g.ldy = ldw; g.sx = g.sy = sA;
    g.C = prec_out; g.ldc = B; g.sc = B * B;
    g.M = B; g.N = B; g.K = B;
    g.upper_only = 1;
    g.xy_lower_tri = 1;
    g.batch = nb;
    WCHK(launch_gemm_tn(st, g));
    for (int32_t b = 0; b < nb; ++b) WCHK(launch_symmetrize_from_upper(st, prec_out + (int64_t)b * B * B, B, B));
  }
  // one copy for everything the host decides on (six small pageable copies were a third of a 48-row block's 0.18 ms)
  std::vector<char> back(p.readback);
  WCHK(hipMemcpyAsync(back.data(), p.rowsum, p.readback, hipMemcpyDeviceToHost, st));
  WCHK(hipStreamSynchronize(st));
  auto at = [&](const void *dev) { return back.data() + ((const char *)dev - (const char *)p.rowsum); };
  const double *rowsum = (const double *)at(p.rowsum), *fro2 = (const double *)at(p.fro2);
  const double *logsd = (const double *)at(p.logsd), *logu = (const double *)at(p.logu);
  const int32_t *info = (const int32_t *)at(p.info), *bad = (const int32_t *)at(p.bad);
  const double cut = std::fabs(svdcut);
  for (int32_t b = 0; b < nb; ++b) {
    double hi = 0.0, tr = 0.0;
    for (int64_t i = 0; i < B; ++i) {
      hi = std::fmax(hi, rowsum[(size_t)(b * B + i)]);
      tr += fro2[(size_t)(b * B + i)];
    }
    if (hi > (double)B) hi = (double)B;            // trace of a correlation matrix
    double lo = 1.0 / tr;                          // rigorous: lambda_min >= 1 / tr inv(corr)
    logdet_out[b] = 2.0 * (logu[b] + logsd[b]);
    int status = 0;
    if (bad[b] || info[b] != 0 || !std::isfinite(tr) || !std::isfinite(logdet_out[b])) {
      status = 2;
      lo = 0.0;
    } else if (cut > 0.0 && !(lo > cut * hi)) {
      // undecided by the bounds: inverse iteration with the factor, u <- Wl^T (Wl u); the estimate
      // approaches lambda_min from above, hence the margin the host applied before (x4)
      const double *Wl = p.Wl + (int64_t)b * sA;
      double *u = p.vec, *t = p.vec + B, *w = p.vec + 2 * B;
      std::vector<double> u0((size_t)B);
      uint64_t s = 0x9E3779B97F4A7C15ull;
      for (int64_t i = 0; i < B; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        u0[(size_t)i] = (double)(s >> 11) / 9007199254740992.0 - 0.5;
      }
      WCHK(hipMemcpyAsync(w, u0.data(), sizeof(double) * B, hipMemcpyHostToDevice, st));
      double nrm2 = 1.0;
      for (int it = 0; it < 40; ++it) {
        WCHK(launch_sumsq(st, w, B, p.partial, p.scal));
        hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, w, p.scal, u, B);
        WCHK(launch_gemv_rows(st, Wl, ldw, B, B, u, t));
        WCHK(launch_colsum_dot(st, Wl, B, ldw, B, 0, p.partial, 256, w, t, 1));
      }
      WCHK(launch_sumsq(st, w, B, p.partial, p.scal));
      WCHK(hipMemcpyAsync(&nrm2, p.scal, sizeof(double), hipMemcpyDeviceToHost, st));
      WCHK(hipStreamSynchronize(st));
      const double est = 1.0 / std::sqrt(nrm2);    // |inv(corr) u| -> 1 / lambda_min
      if (std::isfinite(est) && est > 4.0 * cut * hi) lo = est / 4.0;
      else status = 1;
    }
    status_out[b] = status;
    if (lam_min_out) lam_min_out[b] = lo;
    if (lam_max_out) lam_max_out[b] = hi;
  }
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

// The eigen-mode route (doc/source/overview.rst:1546-1606) for the blocks lsqamd_whiten_blocks hands back, 2 <= B <= 8192:
// copy in -> sdev / correlation -> batched Jacobi eigensolver (eigh_blocks.hip up to 256 rows, eigh_large.hip above) ->
// weights -> inv(C) where wanted.
size_t lsqamd_whiten_eig_work_bytes(int64_t block_size, int32_t n_blocks) try {
  if (block_size < 2 || block_size > kEighLargeMax || n_blocks < 1) return 0;
  return make_eig_plan(block_size, n_blocks, nullptr).bytes + 256;
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_whiten_blocks_eig(void *stream, int64_t B, int32_t nb, const double *cov, double svdcut, double *wt_out,
                             double *prec_out, double *lam_out, double *vec_out, void *dev_work, size_t work_bytes,
                             double *logdet_out, int32_t *modes_out, int32_t *nmod_out, int32_t *sweeps_out,
                             int32_t *status_out) try {
  if (nb < 1 || !cov || !wt_out || !lam_out || !dev_work || !logdet_out || !modes_out || !nmod_out || !status_out)
    return LSQAMD_EINVAL;
  if (B < 2 || B > kEighLargeMax) return LSQAMD_EUNSUPPORTED;       // larger blocks: the caller's LAPACK route
  if (B > kEighBlocksMax && nb > kEighLargeBatchMax) return LSQAMD_EUNSUPPORTED;   // (whiten.py splits such a batch)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char *base = (char *)dev_work;
  const size_t pad = (size_t)((-(intptr_t)base) & 255);
  if (work_bytes < pad) return LSQAMD_ENOMEM;
  EigPlan p = make_eig_plan(B, nb, base + pad);
  if (work_bytes < p.bytes + pad) return LSQAMD_ENOMEM;
  const int64_t ldw = p.ldw, sA = p.strideA;
  // ONE contiguous copy (a pitched copy from pageable memory goes row by row: nb * B small transfers); rows are spread to
  // the leading dimension on the device, through wt_out, which nothing has written yet
  if (ldw == B) {
    WCHK(hipMemcpyAsync(p.A, cov, sizeof(double) * nb * B * B, hipMemcpyDefault, st));
  } else {
    WCHK(hipMemcpyAsync(wt_out, cov, sizeof(double) * nb * B * B, hipMemcpyDefault, st));
    hipLaunchKernelGGL(spread_rows_kernel, dim3((unsigned)B, (unsigned)nb), dim3(256), 0, st, wt_out, B, p.A, ldw, sA);
  }
  WCHK(hipMemsetAsync(p.bad, 0, sizeof(int32_t) * nb, st));
  hipLaunchKernelGGL(sdev_kernel, dim3((unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA, p.sd, p.logsd, p.bad);
  hipLaunchKernelGGL(to_corr_kernel, dim3((unsigned)((B + 3) / 4), (unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA,
                     p.sd, p.rowsum);
  const bool large = B > kEighBlocksMax;
  if (large) WCHK(launch_eigh_large(st, p.A, B, ldw, sA, nb, p.slab, lam_out, p.sweeps, p.status));
  else WCHK(launch_eigh_blocks(st, p.A, B, ldw, sA, nb, p.slab, lam_out, p.sweeps, p.status));
  const int64_t sW = p.strideS ? p.strideS : sA;
  hipLaunchKernelGGL(eig_weights_kernel, dim3((unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA, lam_out, p.sd, p.logsd,
                     p.bad, svdcut, wt_out, prec_out ? p.W : nullptr, ldw, sW, vec_out, p.logdet, p.modes, p.nmod,
                     p.status, p.rs);
  if (large)
    hipLaunchKernelGGL(eig_spread_kernel, dim3((unsigned)B, (unsigned)nb), dim3(256), 0, st, p.A, B, ldw, sA, p.sd, p.rs,
                       svdcut, p.nmod, wt_out, prec_out ? p.W : nullptr, ldw, sW, vec_out);
  if (prec_out) {
    GemmTN g;   // inv(C_b) = Wt_b Wt_b^T = W_b^T W_b (full operands; upper tiles, then mirrored)
    g.X = p.W; g.Y = p.W; g.ldx = g.ldy = ldw; g.sx = g.sy = sW;
    g.C = prec_out; g.ldc = B; g.sc = B * B;
    g.M = B; g.N = B; g.K = B;
    g.upper_only = 1;
    g.batch = nb;
    WCHK(launch_gemm_tn(st, g));
    for (int32_t b = 0; b < nb; ++b) WCHK(launch_symmetrize_from_upper(st, prec_out + (int64_t)b * B * B, B, B));
  }
  std::vector<char> back(p.readback);   // one copy for everything the host reads
  WCHK(hipMemcpyAsync(back.data(), p.logdet, p.readback, hipMemcpyDeviceToHost, st));
  WCHK(hipStreamSynchronize(st));
  auto at = [&](const void *dev) { return back.data() + ((const char *)dev - (const char *)p.logdet); };
  const double *logdet = (const double *)at(p.logdet);
  const int32_t *modes = (const int32_t *)at(p.modes), *nmod = (const int32_t *)at(p.nmod);
  const int32_t *sweeps = (const int32_t *)at(p.sweeps), *status = (const int32_t *)at(p.status);
  for (int32_t b = 0; b < nb; ++b) {
    logdet_out[b] = logdet[b];
    modes_out[b] = modes[b];
    nmod_out[b] = nmod[b];
    if (sweeps_out) sweeps_out[b] = sweeps[b];
    status_out[b] = status[b] == 0 && !std::isfinite(logdet[b]) ? 2 : status[b];
  }
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

}  // extern "C"
