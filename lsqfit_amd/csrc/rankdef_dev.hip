// The GSL form of the rank-deficient covariance (rankdef.hip's pivoted_inverse; gsl_multifit_nlinear_covar(J, 0.0),
// src/lsqfit/_gsl.pyx:704-706) on the device: which columns of G = J^T J survive is found by a blocked Cholesky
// factorisation with diagonal pivoting and a rank exit (LAPACK dpstrf's algorithm, fp64), the inverse of the surviving
// block by the chain the positive-definite covariance uses (potrf_upper -> trtri_upper_to_lower_T -> launch_gemm_tn).
//
// The pivot chain is a dependency chain (pivot j needs the diagonal as all earlier pivots left it), the trailing update a
// rank-64 product; they get different kernels.
//   pstrf_panel_kernel   64 pivots, ONE workgroup of 1024 threads.  The running diagonal and dpstrf's accumulated `dots`
//                        of all n columns live in LDS (16 n bytes); the panel's rows stay in HBM / L2.  Per pivot: argmax
//                        of diag - dots over the remaining columns (a workgroup reduction that carries the index: among
//                        equal entries the LOWEST index wins, pivoted_inverse's strict > scan), the symmetric swap of rows
//                        and columns j <-> pivot over the whole stored matrix (factored rows above included), row j of the
//                        factor  A[j, j+1:] -= A[k0:j, j]^T A[k0:j, j+1:]  scaled by 1 / sqrt(pivot) with the columns
//                        spread over the threads (contiguous row reads), and that row folded into dots.
//   pstrf_trail_kernel   C -= R^T R on the remaining (n - k1)^2 block, R = A[k0:k1, k1:n] (K = 64): a TN product whose two
//                        operands are slices of the same K-major row panel, staged through LDS once per 64 x 64 tile, one
//                        32 x 32 accumulator per wave on v_mfma_f64_16x16x4.  Upper tiles are computed and stored twice,
//                        the second time transposed through LDS, so the next panel's swaps see an exactly symmetric matrix.
// Rank exit without a host round trip: the panel kernel writes the rank and a "done" word, every later launch reads that
// word first and returns; the host enqueues all ceil(n / 64) panel / update pairs.  The matrix is stored in full (both
// triangles valid on entry): rows i < j hold the factor right of the diagonal, rows >= the panel's start hold the symmetric
// trailing matrix as the last update left it (dpstrf's lazy panel: only row j is brought up to date at pivot j).
// The kept block G[S, S], S = perm[:rank], is gathered in pivot order from an untouched copy of G and padded with an
// identity block to n rows, so that the inverse chain runs at the size (and on the kernels) it runs at for a positive-
// definite fit and needs no rank on the host; the scatter puts zeros in the dropped rows and columns.
#include <cfloat>
#include <climits>

#include "fit_state.h"

using namespace lsqamd;

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int PNB = 64;              // pivots per panel = K of the trailing update
constexpr int PT = 1024;             // threads of the panel workgroup
constexpr int64_t kMaxN = 8192;      // 16 n bytes of LDS for diag / dots
constexpr int LDP = 72;              // leading dimension of the staged panel slices
constexpr int LDT = 65;              // ... of the tile on its way to the mirrored store
constexpr size_t kTrailLds = sizeof(double) * 2 * PNB * LDP;
enum { CTL_DONE = 0, CTL_RANK, CTL_STATUS, CTL_WORDS = 4 };
enum { ST_OK = 0, ST_NONFINITE = 1, ST_NOTPD = 2 };

struct Best {
  double v;
  int i, bad;
};
__device__ __forceinline__ void take(Best &a, double v, int i) {
  if (v > a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; }
}
// the largest value of the workgroup and its lowest index, bad or-ed; every thread gets the result
__device__ __forceinline__ Best block_best(Best b, double *rv, int *ri, int *rb) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(b.v, o, 64);
    const int i2 = __shfl_xor(b.i, o, 64), bad2 = __shfl_xor(b.bad, o, 64);
    take(b, v2, i2);
    b.bad |= bad2;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { rv[wave] = b.v; ri[wave] = b.i; rb[wave] = b.bad; }
  __syncthreads();
  Best r = {rv[0], ri[0], rb[0]};
#pragma unroll
  for (int w = 1; w < PT / 64; ++w) {
    take(r, rv[w], ri[w]);
    r.bad |= rb[w];
  }
  __syncthreads();   // the scratch is free for the next call
  return r;
}

// pivots k0 .. min(k0 + 64, n) - 1; grid 1, dynamic LDS 16 n bytes.  k0 = 0 also sets perm, gmax and the control words.
__global__ __launch_bounds__(PT) void pstrf_panel_kernel(double *A, int64_t ld, int n, int k0, int32_t *perm, int32_t *ctl,
                                                         double *gmax) {
  extern __shared__ double lds[];
  double *diag = lds, *dots = lds + n;
  __shared__ double colj[PNB];
  __shared__ double rv[PT / 64];
  __shared__ int ri[PT / 64], rb[PT / 64];
  const int tid = threadIdx.x;
  if (k0 > 0 && ctl[CTL_DONE] != 0) return;
  Best g = {0.0, 0, 0};
  for (int c = tid; c < n; c += PT) {
    const double d = A[c * ld + c];
    diag[c] = d;
    dots[c] = 0.0;
    if (k0 == 0) {
      perm[c] = c;
      if (fabs(d) > g.v) g.v = fabs(d);
    }
  }
  double gm;
  if (k0 == 0) {
    gm = block_best(g, rv, ri, rb).v;     // (a NaN or Inf on the diagonal is met by the first pivot search below)
    if (tid == 0) {
      gmax[0] = gm;
      ctl[CTL_DONE] = ctl[CTL_RANK] = ctl[CTL_STATUS] = 0;
    }
  } else {
    gm = gmax[0];
    __syncthreads();
  }
  const double floor_ = (double)n * DBL_EPSILON * gm;
  const int k1 = k0 + PNB < n ? k0 + PNB : n;
  for (int j = k0; j < k1; ++j) {
    Best b = {-INFINITY, INT_MAX, 0};
    for (int c = j + tid; c < n; c += PT) {
      const double v = diag[c] - dots[c];
      if (!isfinite(v)) b.bad = 1;
      if (v > b.v) { b.v = v; b.i = c; }
    }
    b = block_best(b, rv, ri, rb);
    if (b.bad || !(b.v > floor_)) {      // the same for every thread
      if (tid == 0) {
        ctl[CTL_STATUS] = b.bad ? ST_NONFINITE : ST_OK;
        ctl[CTL_RANK] = j;
        ctl[CTL_DONE] = 1;
      }
      return;
    }
    const int p = b.i;
    if (p != j) {
      double *rj = A + j * ld, *rp = A + p * ld;
      for (int c = tid; c < n; c += PT) {
        const double t = rj[c];
        rj[c] = rp[c];
        rp[c] = t;
      }
      __syncthreads();
      for (int i = tid; i < n; i += PT) {
        double *r = A + i * ld;
        const double t = r[j];
        r[j] = r[p];
        r[p] = t;
      }
      if (tid == 0) {
        const int32_t tp = perm[j];
        perm[j] = perm[p];
        perm[p] = tp;
        double t = diag[j];
        diag[j] = diag[p];
        diag[p] = t;
        t = dots[j];
        dots[j] = dots[p];
        dots[p] = t;
      }
      __syncthreads();
    }
    const double ajj = sqrt(b.v);
    const int nin = j - k0;
    if (tid < nin) colj[tid] = A[(k0 + tid) * ld + j];
    __syncthreads();
    double *rj = A + j * ld;
    const double *pan = A + k0 * ld;
    for (int c = j + 1 + tid; c < n; c += PT) {
      double acc = rj[c];
#pragma unroll 8
      for (int i = 0; i < nin; ++i) acc -= colj[i] * pan[i * ld + c];
      acc /= ajj;
      rj[c] = acc;
      dots[c] += acc * acc;
    }
    if (tid == 0) rj[j] = ajj;
    __syncthreads();
  }
  if (k1 == n && tid == 0) {
    ctl[CTL_RANK] = n;
    ctl[CTL_DONE] = 1;
  }
}

// A[k1:n, k1:n] -= R^T R, R = A[k0:k1, k1:n], k1 = k0 + 64; grid (T, T) 64 x 64 tiles, of which tm <= tn work
__global__ __launch_bounds__(256) void pstrf_trail_kernel(double *A, int64_t ld, int n, int k0, const int32_t *ctl) {
  const int tn = blockIdx.x, tm = blockIdx.y;
  if (tm > tn || ctl[CTL_DONE] != 0) return;
  extern __shared__ double lds[];
  double *As = lds, *Bs = lds + PNB * LDP, *Ts = lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k1 = k0 + PNB, m0 = k1 + tm * 64, c0 = k1 + tn * 64;
  for (int r = wave; r < PNB; r += 4) {
    const double *row = A + (int64_t)(k0 + r) * ld;
    As[r * LDP + lane] = m0 + lane < n ? row[m0 + lane] : 0.0;
    Bs[r * LDP + lane] = c0 + lane < n ? row[c0 + lane] : 0.0;
  }
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1, lm = lane & 15, lk = lane >> 4;
  v4d acc[2][2] = {};
  const double *ab = As + lk * LDP + wm * 32 + lm, *bb = Bs + lk * LDP + wn * 32 + lm;
#pragma unroll
  for (int kk = 0; kk < PNB / 4; ++kk) {
    const double a0 = ab[kk * 4 * LDP], a1 = ab[kk * 4 * LDP + 16];
    const double b0 = bb[kk * 4 * LDP], b1 = bb[kk * 4 * LDP + 16];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
  __syncthreads();   // the slices have been read: Ts takes their place
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * 32 + i * 16 + lk + 4 * r, c = wn * 32 + j * 16 + lm;
        const bool in = m0 + m < n && c0 + c < n;
        double *at = A + (int64_t)(m0 + m) * ld + c0 + c;
        const double v = (in ? *at : 0.0) - acc[i][j][r];
        Ts[m * LDT + c] = v;
        if (in && (tm < tn || m <= c)) *at = v;      // diagonal tiles: the upper half decides
      }
  __syncthreads();
  for (int idx = tid; idx < 64 * 64; idx += 256) {   // the mirror image, rows of the transposed tile contiguous
    const int c = idx >> 6, m = idx & 63;
    if (m0 + m < n && c0 + c < n && (tm < tn || m < c)) A[(int64_t)(c0 + c) * ld + m0 + m] = Ts[m * LDT + c];
  }
}

// M (n x n) = [ G[S, S] in pivot order, 0 ; 0, I ] from the untouched copy of G; grid (ceil(n / 256), n)
__global__ __launch_bounds__(256) void gather_kept_kernel(const double *G, int64_t ldg, int n, const int32_t *perm,
                                                          const int32_t *ctl, double *M, int64_t ldm) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= n) return;
  const int r = ctl[CTL_RANK];
  M[(int64_t)i * ldm + j] = (i < r && j < r) ? G[(int64_t)perm[i] * ldg + perm[j]] : (i == j ? 1.0 : 0.0);
}

// cov[perm[i]][perm[j]] = X[i][j] for i, j < rank, 0 elsewhere; out[0] = rank, out[1] = status
__global__ __launch_bounds__(256) void scatter_cov_kernel(const double *X, int64_t ldx, int n, const int32_t *perm,
                                                          const int32_t *ctl, const int32_t *info, double *cov, int64_t ldc,
                                                          int32_t *out) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  const int r = ctl[CTL_RANK];
  if (i == 0 && j == 0) {
    out[0] = r;
    out[1] = ctl[CTL_STATUS] != ST_OK ? ctl[CTL_STATUS] : (info[0] != 0 ? ST_NOTPD : ST_OK);
  }
  if (j >= n) return;
  cov[(int64_t)perm[i] * ldc + perm[j]] = (i < r && j < r) ? X[(int64_t)i * ldx + j] : 0.0;
}

hipError_t pstrf_enqueue(hipStream_t st, double *A, int64_t n, int64_t ld, int32_t *perm, int32_t *ctl, double *gmax) {
  static PerDeviceOnce lds_set;   // up to 128 KB (panel) and 72 KB (update) of dynamic LDS: above the default limit
  const hipError_t e = lds_set.run([] {
    const hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(pstrf_panel_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * sizeof(double) * kMaxN));
    return e0 != hipSuccess ? e0 : hipFuncSetAttribute(reinterpret_cast<const void *>(pstrf_trail_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrailLds);
  });
  if (e != hipSuccess) return e;
  for (int64_t k0 = 0; k0 < n; k0 += PNB) {
    hipLaunchKernelGGL(pstrf_panel_kernel, dim3(1), dim3(PT), 2 * sizeof(double) * (size_t)n, st, A, ld, (int)n, (int)k0, perm,
                       ctl, gmax);
    const int64_t rest = n - (k0 + PNB);
    if (rest <= 0) break;
    const unsigned T = (unsigned)((rest + 63) / 64);
    hipLaunchKernelGGL(pstrf_trail_kernel, dim3(T, T), dim3(256), kTrailLds, st, A, ld, (int)n, (int)k0, ctl);
  }
  return hipGetLastError();
}

struct PivInv {
  double *G;              // n x n (ldg), both triangles; overwritten by the factor as far as it got
  const double *pristine; // an untouched copy of G (ldw); may be the buffer cov points to
  double *M, *Wl;         // n x n (ldw) each; Wl may be the pristine copy's buffer, or G's
  int64_t n, ldg, ldw, ldc;
  double *chol_work, *gmax, *cov;
  int32_t *info, *perm, *ctl, *out;
};

// everything queued on st, no synchronisation; out[0] = rank, out[1] = status when the stream has drained
hipError_t pivoted_inverse_enqueue(hipStream_t st, const PivInv &a) {
  const int64_t n = a.n;
  hipError_t e = pstrf_enqueue(st, a.G, n, a.ldg, a.perm, a.ctl, a.gmax);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n);
  hipLaunchKernelGGL(gather_kept_kernel, grid, dim3(256), 0, st, a.pristine, a.ldw, (int)n, a.perm, a.ctl, a.M, a.ldw);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = potrf_upper(st, a.M, n, a.ldw, n, a.chol_work, a.info)) != hipSuccess) return e;
  if ((e = trtri_upper_to_lower_T(st, a.M, n, a.ldw, a.chol_work, a.Wl, a.ldw)) != hipSuccess) return e;
  GemmTN g;
  g.X = a.Wl; g.Y = a.Wl; g.ldx = g.ldy = a.ldw;
  g.C = a.M; g.ldc = a.ldw;
  g.M = n; g.N = n; g.K = n;
  g.upper_only = 1;
  g.xy_lower_tri = 1;
  if ((e = launch_gemm_tn(st, g)) != hipSuccess) return e;
  if ((e = launch_symmetrize_from_upper(st, a.M, n, a.ldw)) != hipSuccess) return e;
  hipLaunchKernelGGL(scatter_cov_kernel, grid, dim3(256), 0, st, a.M, a.ldw, (int)n, a.perm, a.ctl, a.info, a.cov, a.ldc, a.out);
  return hipGetLastError();
}

constexpr int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// the leading dimension the fit's own matrices have at n parameters (workspace.hip): the chain runs the kernels it runs there
constexpr int64_t chain_ld(int64_t n) { return n % 128 == 0 ? n + 128 : rup(n + 1, 16); }
size_t op_work_bytes(int64_t n) {
  return n < 1 || n > kMaxN ? 0 : sizeof(double) * (size_t)(2 * n * chain_ld(n) + 8) + potrf_work_bytes(n) + 64;
}

}  // namespace

namespace lsqamd_host {

bool rankdef_dev_supports(int64_t P) { return P >= 1 && P <= kMaxN; }

// covariance_rank_deficient's device route (GSL form): f->cov, the number of dropped directions (> 0) or a negative code
int covariance_rank_deficient_dev(lsqamd_fit *f) {
  const int64_t P = f->P;
  // scratch of O(P) in f->partial (>= 256 (P + 1) doubles, idle outside the reductions of an evaluation)
  double *gmax = f->partial;
  int32_t *ctl = reinterpret_cast<int32_t *>(f->partial + 2);
  int32_t *out = ctl + CTL_WORDS;
  int32_t *perm = out + 4;
  HIPCHK(f, launch_unpack_sym(f->st, f->redbuf, P, f->Wl, f->ldm));    // factored in place
  HIPCHK(f, launch_unpack_sym(f->st, f->redbuf, P, f->cov, f->ldm));   // the copy G[S, S] is gathered from
  f->have_dense_A = false;
  PivInv a;
  a.G = f->Wl; a.pristine = f->cov; a.M = f->M; a.Wl = f->Wl;
  a.n = P; a.ldg = a.ldw = a.ldc = f->ldm;
  a.chol_work = f->chol_work; a.gmax = gmax; a.cov = f->cov;
  a.info = f->info_dev; a.perm = perm; a.ctl = ctl; a.out = out;
  HIPCHK(f, pivoted_inverse_enqueue(f->st, a));
  int32_t res[2] = {0, 0};
  HIPCHK(f, hipMemcpyAsync(res, out, sizeof(res), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  if (res[1] == ST_NONFINITE) return LSQAMD_ENONFINITE;
  if (res[1] != ST_OK || res[0] >= P) return LSQAMD_ENOTPD;   // nothing to drop, or no factor of the kept block: the caller's report
  f->have_cov = true;
  f->logdet = -INFINITY;   // log det of a singular J^T J, as on the host route
  return (int)(P - res[0]);
}

}  // namespace lsqamd_host

extern "C" size_t lsqamd_op_pivoted_inverse_dev_work_bytes(int64_t n) { return op_work_bytes(n); }

extern "C" int lsqamd_op_pivoted_inverse_dev(void *stream, double *G, int64_t n, int64_t ld, double *cov, int64_t ldc,
                                             int32_t *perm, int32_t *rank, double *work, size_t work_bytes) try {
  if (!G || !cov || !perm || !rank || !work || n < 1 || ld < n || ldc < n) return LSQAMD_EINVAL;
  if (n > kMaxN) return LSQAMD_EUNSUPPORTED;
  if (work_bytes < op_work_bytes(n)) return LSQAMD_ENOMEM;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t ldw = chain_ld(n);
  PivInv a;
  a.G = G; a.n = n; a.ldg = ld; a.ldw = ldw; a.ldc = ldc;
  double *W1 = work;
  a.pristine = W1; a.Wl = W1;
  a.M = W1 + n * ldw;
  a.gmax = a.M + n * ldw;
  a.chol_work = a.gmax + 8;
  a.ctl = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(a.chol_work) + potrf_work_bytes(n));
  a.info = a.ctl + CTL_WORDS;
  a.cov = cov; a.perm = perm; a.out = rank;
  if (launch_copy_strided(st, G, ld, W1, ldw, n, n) != hipSuccess) return LSQAMD_EHIP;
  return pivoted_inverse_enqueue(st, a) == hipSuccess ? 0 : LSQAMD_EHIP;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)
