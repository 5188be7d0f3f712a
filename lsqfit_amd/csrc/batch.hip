// Batched LM engine: B independent fits of one shape advance in lockstep, all LM state
// on the device, one round of kernels captured in a hipGraph and replayed.
//
// This is the device counterpart of what lsqfit.empbayes_fit does with a Python loop of
// whole fits (src/lsqfit/_extras.py:153-174, BASELINE.json config 5): the fits share the
// model, x and the data whitening (1/sdev for the 1x1 rows, W_b per correlated block), and
// differ in the prior (mean / sdev per fit), the starting point and -- for simulated /
// bootstrap refits (src/lsqfit/__init__.py:1391-1469,1548-1642) -- the data means; with lsqamdb_set_data_weights also the VALUES
// of the whitening weights (the block structure stays shared): data errors tuned by empbayes_fit (doc/source/eg7.py), bootstrap
// copies from a datalist (src/lsqfit/__init__.py:1625-1642).  Per fit the GSL trust/lm/nielsen/scaling/
// convergence logic of lm_driver.hip is restated as small per-fit device kernels (b_decide,
// b_post); the heavy kernels are the same ones the single-fit path uses, launched with a
// batch dimension: model kernels (grid.y), TN GEMM (grid.z) for J^T J and the Cholesky
// panels/updates, the diagonal-block kernel (one workgroup per fit), back substitution.
//
// One ROUND = one trial step of every still-active fit:
//   build (A_b + mu_b D_b^2 | g_b) -> Cholesky -> back substitution -> x_trial, v.g, |Dv|^2
//   -> residual at x_trial -> chi2_trial -> decide (rho, accept / reject, mu, nu)
//   -> Jacobian, J^T J, J^T f, chi2 at the fit's current x (unchanged if it rejected)
//   -> post (scaling update, niter, convergence tests, retire finished fits).
// Fits that have finished are masked out of every kernel through `active[b]`.
//
// opt.trs = DOGLEG / DDOGLEG / SUBSPACE2D runs another round (round_trs; the branch is taken on the host, LM's launches are
// untouched): step for the current trust radius from the two legs -> residual -> decide (rho, delta) -> commit -> normal
// equations of the fits that moved -> post -> new legs for those fits (legs_all).  Kernels: batch_trs.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "batch.h"
#include "host.h"   // Carver, rup, the pools; through fit_state.h: FAIL, HIPCHK (they need ->err only), jit.h

namespace lsqamd {

// ---- slabs -> packed tiles ---------------------------------------------------------------
__global__ __launch_bounds__(256) void b_finalize_pack_kernel(const double *slabs, int32_t splits,
                                                              int64_t split_stride, int64_t fit_stride,
                                                              int64_t P, int64_t ld, int64_t T, double *apk,
                                                              int64_t apk_stride, const int32_t *active) {
  const int b = blockIdx.z;
  if (!active[b]) return;
  int64_t t = blockIdx.x, tm = 0;
  while (t >= T - tm) { t -= T - tm; ++tm; }
  const int64_t tn = tm + t;
  double *dst = apk + b * apk_stride + (int64_t)blockIdx.x * TBK * TBK;
  const double *src = slabs + b * fit_stride;
  const int c = threadIdx.x & 127;
  for (int rr = (threadIdx.x >> 7); rr < 8; rr += 2) {
    const int r = blockIdx.y * 8 + rr;
    const int64_t i = tm * TBK + r, j = tn * TBK + c;
    double a = 0.0;
    if (i < P && j < P)
      for (int s = 0; s < splits; ++s) a += src[s * split_stride + i * ld + j];
    dst[r * TBK + c] = a;
  }
}

// ---- J^T f, |f|^2 ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void b_colsum_stage1(const double *J, int64_t nrows, int64_t ld,
                                                       int64_t ncols, int64_t rcol, int64_t rpc,
                                                       int64_t j_stride, double *partial,
                                                       int64_t part_stride, const int32_t *active) {
  const int b = blockIdx.z;
  if (!active[b]) return;
  J += b * j_stride;
  partial += b * part_stride;
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r0 = (int64_t)blockIdx.y * rpc;
  int64_t r1 = r0 + rpc;
  if (r1 > nrows) r1 = nrows;
  if (j >= ncols) return;
  const bool two = j + 1 < ncols;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = r0; i < r1; ++i) {
    const double ri = J[i * ld + rcol];
    a0 += J[i * ld + j] * ri;
    if (two) a1 += J[i * ld + j + 1] * ri;
  }
  partial[(int64_t)blockIdx.y * ncols + j] = a0;
  if (two) partial[(int64_t)blockIdx.y * ncols + j + 1] = a1;
}

__global__ __launch_bounds__(256) void b_colsum_stage2(const double *partial, int64_t nchunks,
                                                       int64_t ncols, int64_t part_stride, double *gvec,
                                                       int64_t g_stride, const int32_t *active) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ncols) return;
  const double *p = partial + b * part_stride;
  double a = 0.0;
  for (int64_t c = 0; c < nchunks; ++c) a += p[c * ncols + j];
  gvec[b * g_stride + j] = a;
}

// ---- diagonal prior into (packed A, g, chi2); one workgroup per fit ----------------------------
__global__ __launch_bounds__(256) void b_prior_kernel(int64_t P, int64_t T, const double *prec,
                                                      const double *pmean, const double *x, double *apk,
                                                      int64_t apk_stride, double *gvec, int64_t g_stride,
                                                      const int32_t *active) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!active[b]) return;
  double *A = apk + b * apk_stride, *g = gvec + b * g_stride;
  double c2 = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double w = prec[b * P + j], d = x[b * P + j] - pmean[b * P + j];
    A[pk_diag(j, T)] += w;
    g[j] += w * d;
    c2 += w * d * d;
  }
  c2 = block_sum(c2, sh);
  if (threadIdx.x == 0) g[P] += c2;
}

// ---- dense prior precision shared by the fits (per-fit means): A_b += Lambda, g_b += Lambda d_b,
// chi2_b += d_b^T Lambda d_b with d_b = x_b - pbar_b --------------------------------------------------
__global__ __launch_bounds__(256) void b_prior_matrix_dense_kernel(double *apk, int64_t apk_stride, int64_t P,
                                                                   int64_t T, const double *prec,
                                                                   const int32_t *active) {
  const int b = blockIdx.z;
  if (!active[b]) return;
  int64_t t = blockIdx.x, tm = 0;
  while (t >= T - tm) { t -= T - tm; ++tm; }
  const int64_t tn = tm + t;
  double *dst = apk + b * apk_stride + (int64_t)blockIdx.x * TBK * TBK;
  const int c = threadIdx.x & 127;
  for (int rr = (threadIdx.x >> 7); rr < 8; rr += 2) {
    const int r = blockIdx.y * 8 + rr;
    const int64_t i = tm * TBK + r, j = tn * TBK + c;
    if (i < P && j < P) dst[r * TBK + c] += prec[i * P + j];
  }
}

// tvec[b][j] = sum_k Lambda[j][k] (x_b[k] - pbar_b[k]); one wave per row j
__global__ __launch_bounds__(256) void b_prior_vec_dense_kernel(int64_t P, const double *prec,
                                                                const double *pmean, const double *x,
                                                                double *tvec, const int32_t *active) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= P) return;
  double a = 0.0;
  for (int64_t k = lane; k < P; k += 64) a += prec[j * P + k] * (x[b * P + k] - pmean[b * P + k]);
  a = bsum(a);
  if (lane == 0) tvec[b * P + j] = a;
}

// g_b += t_b ; g_b[P] += d_b . t_b ; one workgroup per fit
__global__ __launch_bounds__(256) void b_prior_apply_kernel(int64_t P, const double *pmean, const double *x,
                                                            const double *tvec, double *gvec, int64_t g_stride,
                                                            const int32_t *active) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!active[b]) return;
  double *g = gvec + b * g_stride;
  double c2 = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double t = tvec[b * P + j];
    g[j] += t;
    c2 += (x[b * P + j] - pmean[b * P + j]) * t;
  }
  c2 = block_sum(c2, sh);
  if (threadIdx.x == 0) g[P] += c2;
}

// ---- trust_init: D, mu, nu, counters -----------------------------------------------------------
__global__ __launch_bounds__(256) void b_init_kernel(int64_t P, int64_t T, const double *apk,
                                                     int64_t apk_stride, const double *gvec,
                                                     int64_t g_stride, double *diag, int scaler,
                                                     BState s) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const double *A = apk + b * apk_stride;
  double mx = -1.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double a = A[pk_diag(j, T)];
    const double cn = sqrt(a > 0.0 ? a : 0.0);
    const double d = (scaler == LSQAMD_SCALE_LEVENBERG) ? 1.0 : (cn == 0.0 ? 1.0 : cn);
    diag[b * P + j] = d;
    mx = fmax(mx, cn / d);
  }
  mx = block_max(mx, sh);
  if (threadIdx.x == 0) {
    s.mu[b] = 1e-3 * mx * mx;
    s.nu[b] = 2;
    s.chi2[b] = gvec[b * g_stride + P];
    s.bad[b] = 0; s.iter[b] = 0; s.nit[b] = 0; s.info[b] = 0; s.status[b] = -2;
    s.active[b] = 1; s.accepted[b] = 0; s.enoprog[b] = 0; s.nfev[b] = 1; s.njev[b] = 1;
  }
}

// ---- M_b = A_b + mu_b D_b^2, column P = g_b ------------------------------------------------------
__global__ __launch_bounds__(256) void b_build_damped_kernel(const double *apk, int64_t apk_stride,
                                                             int64_t P, int64_t T, int64_t ld,
                                                             const double *mu, const double *diag,
                                                             const double *gvec, int64_t g_stride,
                                                             double *M, int64_t m_stride,
                                                             const int32_t *active, int with_damping) {
  const int b = blockIdx.z;
  if (active && !active[b]) return;
  int64_t t = blockIdx.x, tm = 0;
  while (t >= T - tm) { t -= T - tm; ++tm; }
  const int64_t tn = tm + t;
  const double *src = apk + b * apk_stride + (int64_t)blockIdx.x * TBK * TBK;
  double *Mb = M + b * m_stride;
  const double m = with_damping ? mu[b] : 0.0;
  const int c = threadIdx.x & 127;
  for (int rr = (threadIdx.x >> 7); rr < 8; rr += 2) {
    const int r = blockIdx.y * 8 + rr;
    const int64_t i = tm * TBK + r, j = tn * TBK + c;
    if (i < P && j < P) {
      double v = src[r * TBK + c];
      if (i == j) {
        const double d = diag[b * P + i];
        v += m * d * d;
      }
      Mb[i * ld + j] = v;
    }
    if (tn == T - 1 && c == 0 && i < P && gvec) Mb[i * ld + P] = gvec[b * g_stride + i];
  }
}

// y_b = column P of the factored M_b -> yv_b[0..P)
__global__ __launch_bounds__(256) void b_extract_y_kernel(const double *M, int64_t m_stride, int64_t ld,
                                                          int64_t P, double *yv, int64_t y_stride,
                                                          const int32_t *active) {
  const int b = blockIdx.y;
  if (!active[b]) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < P) yv[b * y_stride + j] = M[b * m_stride + j * ld + P];
}

// dx = -v, x_trial = x + dx, v.g, |D v|^2 ; non-finite v marks the factorisation as failed
__global__ __launch_bounds__(256) void b_trial_kernel(int64_t P, const double *yv, int64_t y_stride,
                                                      const double *x, const double *gvec,
                                                      int64_t g_stride, const double *diag, double *dx,
                                                      double *xt, BState s) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!s.active[b]) return;
  const double *v = yv + b * y_stride + P;
  double vg = 0.0, dv2 = 0.0, bad = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double vj = v[j];
    if (!(fabs(vj) < 1.0e300)) bad = 1.0;
    dx[b * P + j] = -vj;
    xt[b * P + j] = x[b * P + j] - vj;
    vg += vj * gvec[b * g_stride + j];
    const double t = diag[b * P + j] * vj;
    dv2 += t * t;
  }
  vg = block_sum(vg, sh);
  dv2 = block_sum(dv2, sh);
  bad = block_sum(bad, sh);
  if (threadIdx.x == 0) {
    s.vg[b] = vg;
    s.dv2[b] = dv2;
    if (bad > 0.0) s.cholinfo[b] = -1;
  }
}

// chi2_trial_b = |r_b|^2 + prior term at x_trial ; two stages
__global__ __launch_bounds__(256) void b_sumsq_stage1(const double *r, int64_t n, int64_t r_stride,
                                                      double *partial, int nparts,
                                                      const int32_t *active) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  if (!active[b]) return;
  const double *rb = r + b * r_stride;
  double a = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = rb[i];
    a += v * v;
  }
  a = block_sum(a, sh);
  if (threadIdx.x == 0) partial[b * nparts + blockIdx.x] = a;
}

__global__ __launch_bounds__(256) void b_sumsq_stage2(const double *partial, int nparts, int64_t P,
                                                      const double *prec, const double *pmean,
                                                      const double *xt, int has_prior, const double *tvec,
                                                      BState s) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!s.active[b]) return;
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += partial[b * nparts + i];
  if (has_prior)
    for (int64_t j = threadIdx.x; j < P; j += 256) {
      const double d = xt[b * P + j] - pmean[b * P + j];
      a += tvec ? d * tvec[b * P + j] : prec[b * P + j] * d * d;   // tvec = Lambda d (dense prior)
    }
  a = block_sum(a, sh);
  if (threadIdx.x == 0) {
    s.chi2t[b] = a;
    s.nfev[b] += 1;
  }
}

// trust_eval_step + nielsen accept/reject, one thread per fit
__global__ void b_decide_kernel(int B, double factor_up, double factor_down, BState s) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  s.moved[b] = 0;
  if (!s.active[b]) return;
  double rho = -1.0;
  if (s.cholinfo[b] == 0) {
    const double normf = sqrt(s.chi2[b]), normf_t = sqrt(s.chi2t[b]);
    if (normf_t < normf) {
      const double u = normf_t / normf;
      const double actual = 1.0 - u * u;
      const double pred = (s.vg[b] + s.mu[b] * s.dv2[b]) / s.chi2[b];
      rho = pred > 0.0 ? actual / pred : -1.0;
    }
  }
  s.accepted[b] = 0;
  s.enoprog[b] = 0;
  if (rho > 0.0) {
    s.accepted[b] = 1;
    s.moved[b] = 1;
    const double bb = 2.0 * rho - 1.0;
    s.mu[b] *= fmax(0.333333333333333, 1.0 - bb * bb * bb);
    s.nu[b] = 2;
    s.bad[b] = 0;
  } else {
    s.mu[b] *= (double)s.nu[b];
    s.nu[b] <<= 1;
    s.bad[b] += 1;
    if (s.bad[b] > 15) {
      s.enoprog[b] = 1;
      s.bad[b] = 0;
    }
  }
}

// accepted fits: x <- x_trial
__global__ __launch_bounds__(256) void b_commit_kernel(int64_t P, double *x, const double *xt, BState s) {
  const int b = blockIdx.y;
  if (!s.active[b] || !s.accepted[b]) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < P) x[b * P + j] = xt[b * P + j];
}

// scaling update, niter, gsl_multifit_nlinear_test, retirement; one workgroup per fit
__global__ __launch_bounds__(256) void b_post_kernel(int64_t P, int64_t T, const double *apk,
                                                     int64_t apk_stride, const double *gvec,
                                                     int64_t g_stride, double *diag, const double *x,
                                                     const double *dx, int scaler, double xtol,
                                                     double gtol, int maxit, BState s) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!s.active[b]) return;
  const bool acc = s.accepted[b] != 0, enp = s.enoprog[b] != 0;
  if (!acc && !enp) return;  // rejected trial: stay in the inner loop
  if (acc) {
    const double *A = apk + b * apk_stride;
    for (int64_t j = threadIdx.x; j < P; j += 256) {
      const double a = A[pk_diag(j, T)];
      const double cn = sqrt(a > 0.0 ? a : 0.0);
      if (scaler == LSQAMD_SCALE_MORE) diag[b * P + j] = fmax(diag[b * P + j], cn);
      else if (scaler == LSQAMD_SCALE_MARQUARDT) diag[b * P + j] = cn == 0.0 ? 1.0 : cn;
    }
  }
  // convergence tests on (dx, x, g, chi2)
  double notx = 0.0, gn = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double xj = x[b * P + j];
    if (!(fabs(dx[b * P + j]) < xtol * xtol + xtol * fabs(xj))) notx = 1.0;
    gn = fmax(gn, fabs(fmax(xj, 1.0) * gvec[b * g_stride + j]));
  }
  notx = block_sum(notx, sh);
  gn = block_max(gn, sh);
  if (threadIdx.x == 0) {
    const double c2 = gvec[b * g_stride + P];
    if (acc) {
      s.chi2[b] = c2;
      s.njev[b] += 1;
    }
    s.nit[b] += 1;
    if (enp && s.iter[b] == 0) {  // no progress on the very first iteration
      s.info[b] = LSQAMD_ENOPROG;
      s.status[b] = LSQAMD_EMAXITER;
      s.active[b] = 0;
      return;
    }
    s.iter[b] += 1;
    int info = 0;
    if (notx == 0.0) info = 1;
    else if (gn <= gtol * fmax(0.5 * s.chi2[b], 1.0)) info = 2;
    if (info) {
      s.info[b] = info;
      s.status[b] = 0;
      s.active[b] = 0;
    } else if (s.iter[b] >= maxit) {
      s.info[b] = 0;
      s.status[b] = LSQAMD_EMAXITER;
      s.active[b] = 0;
    }
  }
}

__global__ void b_count_kernel(int B, BState s) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int c = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) c += s.active[b] ? 1 : 0;
  atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) *s.n_active = cnt;
}

__global__ void b_logdiag_kernel(const double *M, int64_t m_stride, int64_t n, int64_t ld, double *out) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  double a = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += 256) a += log(M[b * m_stride + j * ld + j]);
  a = block_sum(a, sh);
  if (threadIdx.x == 0) out[b] = 2.0 * a;
}

__global__ __launch_bounds__(256) void b_symmetrize_kernel(double *A, int64_t a_stride, int64_t P,
                                                           int64_t ld) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = blockIdx.y;
  double *Ab = A + (int64_t)blockIdx.z * a_stride;
  if (j >= P || j >= i) return;
  Ab[i * ld + j] = Ab[j * ld + i];
}

}  // namespace lsqamd

// ===============================================================================================
using namespace lsqamd;

using lsqamd_host::Carver;
using lsqamd_host::rup;

using EventPairs = std::vector<std::pair<hipEvent_t, hipEvent_t>>;
namespace {
void give_events(EventPairs &v, int dev) {   // back to the pool, filed under the device they were taken on
  for (auto &pr : v) {
    lsqamd_host::event_give(pr.first, dev);
    lsqamd_host::event_give(pr.second, dev);
  }
  v.clear();
}
}  // namespace

struct lsqamdb_fits {
  lsqamd_config cfg;
  lsqamd_options opt;
  int32_t B = 0;
  hipStream_t user_st = nullptr, st = nullptr;
  int dev = -1;                 // the device that was current at lsqamdb_create (recycled streams / events are filed under it)
  std::string err;
  int64_t N = 0, P = 0, ld = 0, ldm = 0, ncols_aug = 0, npk = 0, T = 0, nblk = 0;
  int32_t splits = 1, nparts = 256, nrparts = 64;
  // derived sizes (carve_b): packed tiles per fit; per-fit strides of red = [packed A | g | chi2], of M / Wl / cov, of chol_work
  int64_t ntile = 0, red_stride = 0, m_stride = 0, w_stride = 0;
  double *gvec() const { return red + npk; }   // fit 0's [g | chi2] inside red
  // shared inputs
  double *x = nullptr, *ymean = nullptr, *wdiag = nullptr;
  int64_t ymean_stride = 0;  // 0 shared, N per-fit
  // per-fit whitening weights (lsqamdb_set_data_weights): the caller's device arrays, not copied.  wdiag_b / wt_b are what the
  // kernels read -- the workspace copies of lsqamdb_set_data / _set_blocks with strides 0, or the caller's with strides N and
  // sum_block_sq; tri_b likewise (the caller's flags hold for every fit's block)
  const double *pf_wdiag = nullptr, *pf_wt = nullptr;
  std::vector<int32_t> pf_tri;
  const double *wdiag_b() const { return pf_wdiag ? pf_wdiag : wdiag; }
  const double *wt_b() const { return pf_wdiag ? pf_wt : wt; }
  int64_t wdiag_stride() const { return pf_wdiag ? N : 0; }
  int64_t wt_stride() const { return pf_wdiag ? (int64_t)cfg.sum_block_sq : 0; }
  int32_t tri_b(size_t k) const { return pf_wdiag ? pf_tri[k] : h_tri[k]; }
  // correlated data blocks (shared by the fits)
  uint8_t *in_block = nullptr;
  int64_t *blk_row0 = nullptr, *blk_size = nullptr, *blk_woff = nullptr;
  double *wt = nullptr, *Jraw = nullptr, *r_raw = nullptr;
  std::vector<int64_t> h_row0, h_size, h_modes, h_woff;
  std::vector<int32_t> h_tri;
  bool have_blocks = false;
  int32_t *tape = nullptr;
  double *consts = nullptr;
  int32_t n_tape = 0;
  const void *jit = nullptr;   // the tape compiled (jit.hip); null: the forward-mode interpreter kernel
  // per fit
  double *ptvec = nullptr;  // dense prior: Lambda (x - pbar) per fit
  double *pmean = nullptr, *pprec = nullptr, *px = nullptr, *pxt = nullptr, *dx = nullptr, *diag = nullptr;
  double *r = nullptr, *J = nullptr, *slabs = nullptr, *red = nullptr, *M = nullptr, *chol_work = nullptr;
  double *yv = nullptr, *partial = nullptr, *spart = nullptr, *Wl = nullptr, *cov = nullptr, *logdet = nullptr;
  int32_t *syrk_map = nullptr;
  int32_t syrk_nwork = 0;
  BState s;
  BTrs t;                    // the dogleg family's per-fit state (batch_trs.hip)
  bool have_x = false, have_data = false, have_prior = false, have_tape = false, ran = false, have_cov = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int32_t graph_used = 0, rounds = 0;
  bool one_launch = false, have_cov_from_run = false;   // the last run was one launch (lsqamd_jit_lmb) / it formed the covariances too
  // phase timers (lsqamdb_timing_enable): HIP events around the J^T J launch and the batched factorisation of every round;
  // rounds then run eagerly (events are not recorded into a captured graph)
  bool timing = false;
  EventPairs tm_syrk, tm_chol;
  ~lsqamdb_fits() {
    give_events(tm_syrk, dev);
    give_events(tm_chol, dev);
  }
};

namespace {

// Synchronous copies go through the engine's OWN (non-blocking) stream, never the legacy default stream: a legacy-stream
// operation synchronises with every blocking stream of the process and -- on this runtime -- fails with
// hipErrorStreamCaptureImplicit while ANY thread of the process is capturing a graph, invalidating that thread's capture
// too (found by tests/test_gpu_threads.py: a batch's setters against another handle's step-graph capture).
hipError_t copy_sync(lsqamdb_fits *f, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return hipSuccess;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, f->st);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(f->st);
}

hipError_t copy2d_sync(lsqamdb_fits *f, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                       hipMemcpyKind kind) {
  hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, f->st);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(f->st);
}

size_t carve_b(lsqamdb_fits *f, void *ws, bool dry) {
  const lsqamd_config &c = f->cfg;
  const int64_t N = c.n_data, P = c.n_param, B = f->B;
  f->N = N; f->P = P;
  f->ld = rup(P + 1, 16);
  f->ldm = (P % 128 == 0) ? P + 128 : rup(P + 1, 16);
  f->ncols_aug = (P % 128 == 0) ? P + 128 : P + 1;
  f->npk = packed_doubles(P);
  f->T = (P + 127) / 128;
  f->nblk = f->T;
  f->ntile = f->T * (f->T + 1) / 2; f->red_stride = f->npk + P + 1;
  f->m_stride = P * f->ldm; f->w_stride = f->nblk * 128 * 128;
  {  // split-K: enough workgroups over the whole batch
    const int64_t tiles = f->ntile * B;
    int64_t s = (4096 + tiles - 1) / tiles;
    const int64_t maxs = N / 1024 > 1 ? N / 1024 : 1;
    if (s > maxs) s = maxs;
    if (s > 8) s = 8;
    if (s < 1) s = 1;
    if (const char *e = getenv("LSQAMD_BATCH_SPLITS")) {  // developer knob
      const int v = atoi(e);
      if (v >= 1 && v <= 16) s = v;
    }
    f->splits = (int32_t)s;
  }
  f->nparts = 64; f->nrparts = 32;
  Carver cv(ws, 0, dry);
  f->x = cv.take<double>(N * (c.n_x > 0 ? c.n_x : 1));
  f->ymean = cv.take<double>(B * N);
  f->wdiag = cv.take<double>(N);
  f->in_block = cv.take<uint8_t>(N);
  f->blk_row0 = cv.take<int64_t>(c.n_blocks);
  f->blk_size = cv.take<int64_t>(c.n_blocks);
  f->blk_woff = cv.take<int64_t>(c.n_blocks);
  f->wt = cv.take<double>(c.sum_block_sq);
  f->Jraw = cv.take<double>(c.n_blocks > 0 ? B * N * f->ld : 1);
  f->r_raw = cv.take<double>(c.n_blocks > 0 ? B * N : 1);
  f->tape = cv.take<int32_t>(1024);
  f->consts = cv.take<double>(256);
  f->pmean = cv.take<double>(B * P);
  f->pprec = cv.take<double>(c.prior_dense ? P * P : B * P);
  f->ptvec = cv.take<double>(c.prior_dense ? B * P : 1);
  f->px = cv.take<double>(B * P);
  f->pxt = cv.take<double>(B * P);
  f->dx = cv.take<double>(B * P);
  f->diag = cv.take<double>(B * P);
  f->r = cv.take<double>(B * N);
  f->J = cv.take<double>(B * N * f->ld);
  f->slabs = cv.take<double>(B * f->splits * f->m_stride);
  f->red = cv.take<double>(B * f->red_stride);
  f->M = cv.take<double>(B * f->m_stride);
  f->chol_work = cv.take<double>(B * f->w_stride);
  f->yv = cv.take<double>(B * 2 * P);
  f->partial = cv.take<double>(B * f->nparts * (P + 1));
  f->spart = cv.take<double>(B * f->nrparts);
  f->Wl = cv.take<double>(B * f->m_stride);
  f->cov = cv.take<double>(B * f->m_stride);
  f->logdet = cv.take<double>(B);
  f->s.mu = cv.take<double>(B); f->s.chi2 = cv.take<double>(B); f->s.chi2t = cv.take<double>(B);
  f->s.vg = cv.take<double>(B); f->s.dv2 = cv.take<double>(B);
  f->s.nu = cv.take<int32_t>(B); f->s.bad = cv.take<int32_t>(B); f->s.iter = cv.take<int32_t>(B);
  f->s.nit = cv.take<int32_t>(B); f->s.info = cv.take<int32_t>(B); f->s.status = cv.take<int32_t>(B);
  f->s.active = cv.take<int32_t>(B); f->s.accepted = cv.take<int32_t>(B); f->s.enoprog = cv.take<int32_t>(B);
  f->s.cholinfo = cv.take<int32_t>(B); f->s.nfev = cv.take<int32_t>(B); f->s.njev = cv.take<int32_t>(B);
  f->s.n_active = cv.take<int32_t>(4);
  f->s.moved = cv.take<int32_t>(B);
  f->syrk_nwork = (int32_t)syrk_work_count(P, f->splits);
  f->syrk_map = cv.take<int32_t>(4 * (int64_t)f->syrk_nwork);
  // dogleg family (after everything plain LM uses: its layout does not move)
  f->t.rec = cv.take<double>(B * TR_COUNT);
  f->t.w = cv.take<double>(B * P); f->t.aw = cv.take<double>(B * P);
  f->t.dx_sd = cv.take<double>(B * P); f->t.dx_gn = cv.take<double>(B * P);
  f->t.part = cv.take<double>(B * symv_packed_partials(P));
  f->t.gn_failed = cv.take<int32_t>(B); f->t.lmask = cv.take<int32_t>(B);
  return cv.off;
}

int check_cfg_b(const lsqamd_config *c, int32_t B) {
  if (!c || c->abi_version != LSQAMD_ABI_VERSION || B < 1) return LSQAMD_EINVAL;
  if (c->n_data < 1 || c->n_param < 1) return LSQAMD_EINVAL;
  if (c->n_blocks < 0) return LSQAMD_EUNSUPPORTED;
  if (c->model < LSQAMD_MODEL_COSMIX || c->model > LSQAMD_MODEL_IDENTITY) return LSQAMD_EINVAL;
  if (c->model == LSQAMD_MODEL_TAPE && c->n_param > LSQAMD_TAPE_MAX_PARAM) return LSQAMD_EINVAL;
  if ((c->model == LSQAMD_MODEL_COSMIX || c->model == LSQAMD_MODEL_MULTIEXP) && (c->n_param & 1))
    return LSQAMD_EINVAL;
  return 0;
}

ModelArgs model_args_b(const lsqamdb_fits *f, const double *p) {
  ModelArgs m;
  m.model = f->cfg.model;
  m.n_data = f->N; m.n_param = f->P;
  m.n_x = f->cfg.n_x > 0 ? f->cfg.n_x : 1;
  m.x = f->x; m.ymean = f->ymean; m.wdiag = f->wdiag_b();
  m.ymean_stride = f->ymean_stride; m.wdiag_stride = f->wdiag_stride();
  m.in_block = f->cfg.n_blocks > 0 ? f->in_block : nullptr;
  m.p = p; m.tape = f->tape; m.n_tape = f->n_tape; m.consts = f->consts;
  m.n_batch = f->B; m.p_stride = f->P; m.batch_active = f->s.active;
  m.jit = f->jit;
  return m;
}

struct Bracket {   // HIP-event bracket around one launch while the handle's timers are on (lsqamd_host::Scope's counterpart)
  lsqamdb_fits *f;
  EventPairs &into;
  hipEvent_t a = nullptr, b = nullptr;
  Bracket(lsqamdb_fits *fits, EventPairs &list, bool on = true) : f(fits), into(list) {
    if (!on || !f->timing) return;
    a = lsqamd_host::event_take();
    b = lsqamd_host::event_take();
    (void)hipEventRecord(a, f->st);
  }
  ~Bracket() {   // filed whether or not the launch went through: the list owns the pair from here on
    if (!a) return;
    (void)hipEventRecord(b, f->st);
    into.emplace_back(a, b);
  }
};

// the whitened Jacobian (its last column: the residual) of every fit flagged in `mask` at its current x
int jacobian_all(lsqamdb_fits *f, const int32_t *mask) {
  const int64_t P = f->P, N = f->N;
  ModelArgs m = model_args_b(f, f->px);
  m.batch_active = mask;
  m.out_stride = N * f->ld;
  HIPCHK(f, launch_jacobian_ex(f->st, m, f->J, f->cfg.n_blocks > 0 ? f->Jraw : nullptr, f->ld));
  // block rows: J_b <- W_b . Jraw_b for every fit (batch = fits; X stride 0 when W is shared, else sum_block_sq -- an odd
  // stride leaves the 16-byte loads to launch_gemm_tn's alignment test)
  for (size_t k = 0; k < f->h_size.size(); ++k) {
    const int64_t Bk = f->h_size[k];
    GemmTN w;
    w.X = f->wt_b() + f->h_woff[k]; w.ldx = Bk; w.sx = f->wt_stride();
    w.Y = f->Jraw + f->h_row0[k] * f->ld; w.ldy = f->ld; w.sy = N * f->ld;
    w.C = f->J + f->h_row0[k] * f->ld; w.ldc = f->ld; w.sc = N * f->ld;
    w.M = Bk; w.N = P + 1; w.K = Bk;
    w.x_upper_tri = f->tri_b(k);
    w.batch = (int32_t)f->B; w.batch_active = mask;
    HIPCHK(f, launch_gemm_tn(f->st, w));
  }
  return 0;
}

// J^T J -> packed tiles, J^T f and |f|^2 -> [g | chi2], from the Jacobian jacobian_all left
int product_all(lsqamdb_fits *f, const int32_t *mask) {
  const int64_t P = f->P, N = f->N;
  const unsigned B = (unsigned)f->B;
  GemmTN g;
  g.X = f->J; g.Y = f->J; g.ldx = g.ldy = f->ld; g.sx = g.sy = N * f->ld;
  g.C = f->slabs; g.ldc = f->ldm; g.sc = (int64_t)f->splits * f->m_stride;
  g.M = P; g.N = P; g.K = N;
  g.upper_only = 1; g.splits = f->splits; g.split_stride = f->m_stride;
  g.work_map = f->syrk_map; g.n_work = f->syrk_nwork;
  g.batch = (int32_t)B; g.batch_active = mask;
  // J^T f and chi2 from the diagonal tiles of the same launch when it is the kernel that can (P a multiple of 128):
  // partial[(b * splits + split)][P + 1]   (splits <= 16 <= nparts)
  g.colsum_out = f->partial; g.colsum_ld = P + 1; g.colsum_rcol = P;
  const bool syrk_colsum = gemm_tn_fuses_colsum(g);
  if (!syrk_colsum) g.colsum_out = nullptr;
  {
    Bracket tb(f, f->tm_syrk);
    HIPCHK(f, launch_gemm_tn(f->st, g));
  }
  hipLaunchKernelGGL(b_finalize_pack_kernel, dim3((unsigned)f->ntile, 16, B), dim3(256), 0, f->st, f->slabs, f->splits,
                     f->m_stride, (int64_t)f->splits * f->m_stride, P, f->ldm, f->T, f->red, f->red_stride, mask);
  int64_t nchunks = f->splits, part_stride = (int64_t)f->splits * (P + 1);
  if (!syrk_colsum) {
    nchunks = f->nparts;
    if (nchunks > N) nchunks = N;
    const int64_t rpc = (N + nchunks - 1) / nchunks;
    nchunks = (N + rpc - 1) / rpc;
    part_stride = (int64_t)f->nparts * (P + 1);
    hipLaunchKernelGGL(b_colsum_stage1, dim3((unsigned)((P + 1 + 511) / 512), (unsigned)nchunks, B), dim3(256), 0, f->st, f->J,
                       N, f->ld, P + 1, P, rpc, N * f->ld, f->partial, part_stride, mask);
  }
  hipLaunchKernelGGL(b_colsum_stage2, dim3((unsigned)((P + 1 + 255) / 256), B), dim3(256), 0, f->st, f->partial, nchunks, P + 1,
                     part_stride, f->gvec(), f->red_stride, mask);
  return 0;
}

// Lambda (x - pbar) of every fit flagged in `mask` (dense shared prior) -> f->ptvec
void prior_vec_dense(lsqamdb_fits *f, const double *x, const int32_t *mask) {
  hipLaunchKernelGGL(b_prior_vec_dense_kernel, dim3((unsigned)((f->P + 3) / 4), (unsigned)f->B), dim3(256), 0, f->st, f->P,
                     f->pprec, f->pmean, x, f->ptvec, mask);
}

// Jacobian, J^T J (packed), J^T f, chi2, then the prior's share of all three, for every fit flagged in `mask` at its current x
// (inside a round: the fits whose trial was accepted -- a rejected trial leaves x, J and the sums as they are)
int normal_all(lsqamdb_fits *f, const int32_t *mask) {
  int rc = jacobian_all(f, mask);
  if (rc || (rc = product_all(f, mask))) return rc;
  const int64_t P = f->P;
  const unsigned B = (unsigned)f->B;
  if (f->cfg.has_prior && f->cfg.prior_dense) {
    hipLaunchKernelGGL(b_prior_matrix_dense_kernel, dim3((unsigned)f->ntile, 16, B), dim3(256), 0, f->st, f->red,
                       f->red_stride, P, f->T, f->pprec, mask);
    prior_vec_dense(f, f->px, mask);
    hipLaunchKernelGGL(b_prior_apply_kernel, dim3(B), dim3(256), 0, f->st, P, f->pmean, f->px, f->ptvec, f->gvec(),
                       f->red_stride, mask);
  } else if (f->cfg.has_prior) {
    hipLaunchKernelGGL(b_prior_kernel, dim3(B), dim3(256), 0, f->st, P, f->T, f->pprec, f->pmean, f->px, f->red,
                       f->red_stride, f->gvec(), f->red_stride, mask);
  }
  HIPCHK(f, hipGetLastError());
  return 0;
}

// residual and chi2 (+ prior term) of every active fit at its trial point
int trial_chi2_all(lsqamdb_fits *f) {
  const int64_t P = f->P, N = f->N, B = f->B;
  ModelArgs m = model_args_b(f, f->pxt);
  m.out_stride = N;
  HIPCHK(f, launch_residual_ex(f->st, m, f->r, f->cfg.n_blocks > 0 ? f->r_raw : nullptr));
  if (f->cfg.n_blocks > 0)
    HIPCHK(f, launch_block_whiten_vec(f->st, f->wt_b(), f->blk_row0, f->blk_size, f->blk_woff, f->cfg.n_blocks,
                                      f->cfg.max_block, f->r_raw, f->r, (int32_t)B, N, f->s.active, INT64_MAX,
                                      f->wt_stride()));
  hipLaunchKernelGGL(b_sumsq_stage1, dim3((unsigned)f->nrparts, (unsigned)B), dim3(256), 0, f->st, f->r, N, N,
                     f->spart, f->nrparts, f->s.active);
  const bool dense_prior = f->cfg.has_prior && f->cfg.prior_dense;
  if (dense_prior) prior_vec_dense(f, f->pxt, f->s.active);
  hipLaunchKernelGGL(b_sumsq_stage2, dim3((unsigned)B), dim3(256), 0, f->st, f->spart, f->nrparts, P, f->pprec,
                     f->pmean, f->pxt, f->cfg.has_prior, dense_prior ? f->ptvec : nullptr, f->s);
  return 0;
}

// (A_b + mu_b D_b^2 | g_b) -- with_damping = 0: (A_b | g_b) -- built, factored and back-substituted for every fit flagged in
// `mask`: v_b lands in f->yv[b][P..2P), a failed pivot in s.cholinfo[b].  timed: the factorisation counts for the cholesky timer
int factor_and_solve(lsqamdb_fits *f, const int32_t *mask, int with_damping, bool timed) {
  const int64_t P = f->P;
  const int32_t B = f->B;
  hipLaunchKernelGGL(b_build_damped_kernel, dim3((unsigned)f->ntile, 16, (unsigned)B), dim3(256), 0, f->st, f->red,
                     f->red_stride, P, f->T, f->ldm, f->s.mu, f->diag, f->gvec(), f->red_stride, f->M, f->m_stride, mask,
                     with_damping);
  {
    Bracket tb(f, f->tm_chol, timed);
    HIPCHK(f, potrf_upper_batched(f->st, f->M, P, f->ldm, f->ncols_aug, f->chol_work, f->s.cholinfo, B, f->m_stride,
                                  f->w_stride, mask));
  }
  hipLaunchKernelGGL(b_extract_y_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)B), dim3(256), 0, f->st, f->M,
                     f->m_stride, f->ldm, P, f->yv, 2 * P, mask);
  HIPCHK(f, backsolve_upper_batched(f->st, f->M, P, f->ldm, f->chol_work, f->yv, B, f->m_stride, f->w_stride, 2 * P, mask));
  return 0;
}

// the tail of a round of either kind: the accepted fits move, get new normal equations, then the scaling update, niter and
// the convergence tests of every active fit
int commit_normal_post(lsqamdb_fits *f) {
  const int64_t P = f->P;
  const unsigned B = (unsigned)f->B;
  hipLaunchKernelGGL(b_commit_kernel, dim3((unsigned)((P + 255) / 256), B), dim3(256), 0, f->st, P, f->px, f->pxt, f->s);
  const int rc = normal_all(f, f->s.moved);
  if (rc) return rc;
  hipLaunchKernelGGL(b_post_kernel, dim3(B), dim3(256), 0, f->st, P, f->T, f->red, f->red_stride, f->gvec(), f->red_stride,
                     f->diag, f->px, f->dx, f->opt.scaler, f->opt.xtol, f->opt.gtol, f->opt.maxit, f->s);
  return 0;
}

int round_all(lsqamdb_fits *f) {
  const int64_t P = f->P, B = f->B;
  int rc = factor_and_solve(f, f->s.active, 1, true);
  if (rc) return rc;
  hipLaunchKernelGGL(b_trial_kernel, dim3((unsigned)B), dim3(256), 0, f->st, P, f->yv, 2 * P, f->px, f->gvec(),
                     f->red_stride, f->diag, f->dx, f->pxt, f->s);
  if ((rc = trial_chi2_all(f))) return rc;
  hipLaunchKernelGGL(b_decide_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, f->st, (int)B,
                     f->opt.factor_up, f->opt.factor_down, f->s);
  if ((rc = commit_normal_post(f))) return rc;
  hipLaunchKernelGGL(b_count_kernel, dim3(1), dim3(256), 0, f->st, (int)B, f->s);
  HIPCHK(f, hipGetLastError());
  return 0;
}

// ---- the dogleg family (opt.trs = DOGLEG / DDOGLEG / SUBSPACE2D; kernels in batch_trs.hip) ------------------------------
// The two legs of every fit flagged in `mask` at its current (A, g, D): w = D^-2 g, ONE symmetric product for w^T A w, the
// Gauss-Newton point from the undamped normal equations (the same build / factorisation / back substitution as an LM trial,
// with mu = 0; not counted by the cholesky timer), then the scalars the step kernel works from.
int legs_all(lsqamdb_fits *f, const int32_t *mask) {
  const int64_t P = f->P;
  const int32_t B = f->B;
  HIPCHK(f, launch_trs_grad(f->st, P, B, f->gvec(), f->red_stride, f->diag, f->t, mask));
  HIPCHK(f, launch_symv_packed(f->st, f->red, f->red_stride, P, B, f->t.w, P, f->t.part, f->t.aw, P, f->t.rec + TR_WAW,
                               TR_COUNT, mask));
  const int rc = factor_and_solve(f, mask, 0, false);
  if (rc) return rc;
  HIPCHK(f, launch_trs_legs(f->st, P, B, f->opt.trs, f->gvec(), f->red_stride, f->diag, f->yv + P, 2 * P, f->s.cholinfo, f->t,
                            mask));
  return 0;
}

// One round of the family: the step for the current delta -> residual and chi2 there -> rho, delta, accept / reject ->
// the accepted fits move, get new normal equations, the scaling update and the convergence tests (b_post_kernel, as in LM)
// -> new legs for the fits that moved and go on.  A fit that rejected keeps its legs: no product, no factorisation.
int round_trs(lsqamdb_fits *f) {
  const int32_t B = f->B;
  HIPCHK(f, launch_trs_step(f->st, f->P, B, f->opt.trs, f->px, f->pxt, f->dx, f->t, f->s.active));
  int rc = trial_chi2_all(f);
  if (rc) return rc;
  HIPCHK(f, launch_trs_decide(f->st, B, f->opt.factor_up, f->opt.factor_down, f->s, f->t));
  if ((rc = commit_normal_post(f))) return rc;
  HIPCHK(f, launch_trs_mask(f->st, B, f->s, f->t));
  if ((rc = legs_all(f, f->t.lmask))) return rc;
  hipLaunchKernelGGL(b_count_kernel, dim3(1), dim3(256), 0, f->st, (int)B, f->s);
  HIPCHK(f, hipGetLastError());
  return 0;
}

int round_any(lsqamdb_fits *f) { return f->opt.trs == LSQAMD_TRS_LM ? round_all(f) : round_trs(f); }

// ---- the stages of lsqamdb_run -------------------------------------------------------------------------------------
// does the device allocation p points into reach n doubles beyond p?  (what the engine can know of a caller's array: weights
// made for fewer fits than the handle runs would be read past their end.  Memory the runtime cannot name a range for --
// a pool's sub-allocation is judged by its segment -- is taken on trust)
bool holds_doubles(const double *p, int64_t n) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<double *>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return true;
  }
  const char *lo = static_cast<const char *>(static_cast<const void *>(base));
  const char *q = reinterpret_cast<const char *>(p);
  return q >= lo && (size_t)(q - lo) + sizeof(double) * (size_t)n <= size;
}

int inputs_ready(lsqamdb_fits *f) {
  if (!f->have_data || (f->cfg.has_prior && !f->have_prior) || (f->cfg.n_blocks > 0 && !f->have_blocks) ||
      (f->cfg.model != LSQAMD_MODEL_IDENTITY && !f->have_x) || (f->cfg.model == LSQAMD_MODEL_TAPE && !f->have_tape))
    FAIL(f, LSQAMD_EINVAL, "run: inputs missing");
  if (f->pf_wdiag) {   // per-fit weights: the caller's arrays must hold every fit of THIS batch
    if (f->cfg.n_blocks > 0 && !f->pf_wt) FAIL(f, LSQAMD_EINVAL, "run: per-fit weights without wt, but the config has blocks");
    if (!holds_doubles(f->pf_wdiag, (int64_t)f->B * f->N) ||
        (f->cfg.n_blocks > 0 && !holds_doubles(f->pf_wt, (int64_t)f->B * f->cfg.sum_block_sq)))
      FAIL(f, LSQAMD_EINVAL, "run: the per-fit weights were set for another number of fits (need %d)", (int)f->B);
  }
  return 0;
}

struct RunSpan {   // the two events a run's device time is read from: every return path gives them back
  lsqamdb_fits *f;
  hipEvent_t e0 = lsqamd_host::event_take(), e1 = lsqamd_host::event_take();
  ~RunSpan() { lsqamd_host::event_give(e0, f->dev); lsqamd_host::event_give(e1, f->dev); }
};

// every fit active (the host's vector is pageable: the stream is waited for before it goes)
int activate_all(lsqamdb_fits *f) {
  std::vector<int32_t> ones((size_t)f->B, 1);
  HIPCHK(f, hipMemcpyAsync(f->s.active, ones.data(), sizeof(int32_t) * f->B, hipMemcpyHostToDevice, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
}

// the state either route starts from: x = p0, every fit active
int start_at(lsqamdb_fits *f, const double *p0) {
  HIPCHK(f, hipMemcpyAsync(f->px, p0, sizeof(double) * f->B * f->P, hipMemcpyHostToDevice, f->st));
  return activate_all(f);
}

// Small fits (a compiled formula, <= 12 parameters, <= 4096 uncorrelated rows or <= 256 with covariance blocks): every
// fit of the batch is ONE workgroup of ONE launch (jit.hip lsqamd_jit_lmb -- the loop of the single-fit kernel, lm_driver.hip
// run_one_launch) instead of ~20 lockstep launches per round.  -> 1: done (rounds, one_launch, have_cov_from_run set); 0: not
// this batch's route, or the kernel met an irregular fit and the lockstep engine runs the whole batch from the start (p0
// again, every fit active); < 0: error.  LSQAMD_ONE_LAUNCH_FIT=0 disables (read per call).
int try_one_launch(lsqamdb_fits *f, const double *p0) {
  f->one_launch = false;
  const int64_t P = f->P, B = f->B;
  const char *e = getenv("LSQAMD_ONE_LAUNCH_FIT");
  if (e && e[0] == '0') return 0;
  const lsqamd_jit::Kernel *k = static_cast<const lsqamd_jit::Kernel *>(f->jit);
  if (!lsqamd_jit::has_batch_fit_kernel(k) || P > lsqamd_jit::FIT_MAX_P || f->N < 1 ||
      f->N > lsqamd_jit::fit_row_limit(k, f->cfg.n_blocks != 0) || f->cfg.n_blocks > 64) return 0;
  if (f->opt.maxit < 1 || f->opt.maxit > 20000 || f->opt.trs != LSQAMD_TRS_LM) return 0;
  lsqamd_jit::FitArgs a;
  a.x = f->x; a.ymean = f->ymean; a.wdiag = f->wdiag_b(); a.n_data = f->N;
  a.in_block = f->in_block; a.wt = f->wt_b();
  a.blk_row0 = reinterpret_cast<const long long *>(f->blk_row0); a.blk_size = reinterpret_cast<const long long *>(f->blk_size);
  a.blk_woff = reinterpret_cast<const long long *>(f->blk_woff); a.n_blocks = f->cfg.n_blocks;
  a.p0 = f->px; a.p = f->px; a.p_trial = f->pxt; a.dscale = f->diag; a.apk = f->red; a.gvec = f->gvec();
  a.v_out = f->dx; a.coln2 = nullptr; a.st = nullptr;
  a.prior_prec = f->cfg.has_prior ? f->pprec : nullptr; a.prior_mean = f->cfg.has_prior ? f->pmean : nullptr;
  a.prior_dense = f->cfg.prior_dense; a.scaler = f->opt.scaler; a.maxit = f->opt.maxit; a.watch = 0;
  a.xtol = f->opt.xtol; a.gtol = f->opt.gtol; a.factor_up = f->opt.factor_up; a.factor_down = f->opt.factor_down;
  a.hostptr_bits = 0.0; a.cov = f->cov; a.ldc = f->ldm; a.want_cov = 1; a.pad_ = 0;
  a.host = f->chol_work;                       // (free until a covariance is asked for: 16384 doubles per fit)
  a.pub = nullptr; a.seq = 0;                  // (the batch's results are copied after a stream synchronisation)
  lsqamd_jit::FitBatch bt;
  bt.ymean_stride = f->ymean_stride; bt.prec_stride = f->cfg.prior_dense ? 0 : P; bt.tile_stride = f->red_stride;
  bt.cov_stride = f->m_stride; bt.scratch_stride = f->w_stride;
  bt.wdiag_stride = f->wdiag_stride(); bt.wt_stride = f->wt_stride();
  bt.logdet = f->logdet; bt.mu = f->s.mu; bt.chi2 = f->s.chi2;
  bt.nit = f->s.nit; bt.info = f->s.info; bt.status = f->s.status; bt.nfev = f->s.nfev; bt.njev = f->s.njev;
  bt.active = f->s.active; bt.reason = f->s.bad;
  HIPCHK(f, lsqamd_jit::launch_fit_batch(k, f->st, a, bt, (int)B));
  std::vector<int32_t> reason((size_t)B, 0);
  HIPCHK(f, hipMemcpyAsync(reason.data(), f->s.bad, sizeof(int32_t) * B, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  bool all_done = true, all_cov = true;
  for (int32_t r : reason) {
    all_done = all_done && (r == 1 || r == 3);
    all_cov = all_cov && r == 1;
  }
  if (!all_done) return start_at(f, p0);
  f->one_launch = true;
  f->rounds = 1;
  f->graph_used = 0;
  f->have_cov_from_run = all_cov;
  return 1;
}

// the lockstep engine's state at p0: normal equations, D, mu (b_init_kernel), for the dogleg family its trust radius and the
// legs; no graph from an earlier run (kernel arguments -- tolerances, maxit, factors -- are baked into graph nodes)
int start_lockstep(lsqamdb_fits *f) {
  int rc = normal_all(f, f->s.active);
  if (rc) return rc;
  hipLaunchKernelGGL(b_init_kernel, dim3((unsigned)f->B), dim3(256), 0, f->st, f->P, f->T, f->red, f->red_stride, f->gvec(),
                     f->red_stride, f->diag, f->opt.scaler, f->s);
  if (f->opt.trs != LSQAMD_TRS_LM) {
    HIPCHK(f, launch_trs_init(f->st, f->P, f->B, f->diag, f->px, f->t));
    if ((rc = legs_all(f, f->s.active))) return rc;
  }
  f->rounds = 0;
  f->graph_used = 0;
  if (f->gexec) { (void)hipGraphExecDestroy(f->gexec); f->gexec = nullptr; }
  if (f->graph) { (void)hipGraphDestroy(f->graph); f->graph = nullptr; }
  return 0;
}

// One attempt at capturing a round into f->gexec (nothing runs: the caller launches it).  f->gexec stays null when the capture
// or the instantiation failed -- the caller goes on eagerly, on a stream that has been reset.  Non-zero: a launch of the round
// failed although the capture itself came through.
int capture_round(lsqamdb_fits *f) {
  if (hipStreamBeginCapture(f->st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    const int rc = round_any(f);
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(f->st, &gr);
    // a capture another thread's activity invalidated makes the captured launches fail too: that is a failed CAPTURE
    // (nothing ran, nothing changed on the device), not a failed round -- the caller's round runs eagerly
    if (rc && e == hipSuccess) return rc;
    if (e == hipSuccess && gr && hipGraphInstantiate(&f->gexec, gr, nullptr, nullptr, 0) == hipSuccess) {
      f->graph = gr;
    } else {
      if (gr) (void)hipGraphDestroy(gr);
      f->gexec = nullptr;
      capture_reset(f->st);      // (an invalidated capture leaves the stream unusable until it is reset: common.h)
    }
  }
  (void)hipGetLastError();
  return 0;
}

// the per-fit scalars lie one after the other in the workspace (carve_b: s.mu .. s.njev): ONE copy instead of seven
int write_summaries(lsqamdb_fits *f, lsqamd_summary *summaries, float ms) {
  const int64_t B = f->B;
  const char *lo = reinterpret_cast<const char *>(f->s.mu), *hi = reinterpret_cast<const char *>(f->s.njev + B);
  std::vector<char> span((size_t)(hi - lo));
  HIPCHK(f, copy_sync(f, span.data(), lo, span.size(), hipMemcpyDeviceToHost));
  auto at = [&](const auto *dev) {   // the host copy of a device array inside the span
    return reinterpret_cast<decltype(dev)>(span.data() + (reinterpret_cast<const char *>(dev) - lo));
  };
  const double *mu = at(f->s.mu), *chi2 = at(f->s.chi2);
  const int32_t *nit = at(f->s.nit), *info = at(f->s.info), *status = at(f->s.status), *nfev = at(f->s.nfev), *njev = at(f->s.njev);
  for (int64_t b = 0; b < B; ++b) {
    lsqamd_summary &s = summaries[b];
    std::memset(&s, 0, sizeof(s));
    s.status = status[b] == -2 ? LSQAMD_EMAXITER : status[b];
    s.info = info[b];
    s.stopping_criterion = (info[b] >= 0 && info[b] <= 3) ? info[b] : (info[b] == 27 ? 4 : 0);
    s.nit = nit[b]; s.nfev = nfev[b]; s.njev = njev[b]; s.ntrial = nfev[b] - 1;
    s.chi2 = chi2[b]; s.mu = mu[b];
    s.logdet_jtj = NAN;
    s.t_run_ms = ms;
    s.t_setup_ms = (double)f->graph_used;  // rounds replayed from the captured graph
  }
  return 0;
}

}  // namespace

extern "C" {

size_t lsqamdb_workspace_bytes(const lsqamd_config *cfg, int32_t n_fits) try {
  if (check_cfg_b(cfg, n_fits) != 0) return 0;
  lsqamdb_fits tmp;
  tmp.cfg = *cfg;
  tmp.B = n_fits;
  return carve_b(&tmp, nullptr, true);
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamdb_create(const lsqamd_config *cfg, int32_t n_fits, void *dev_workspace, size_t workspace_bytes,
                   void *stream, lsqamdb_fits **out) try {
  if (!out) return LSQAMD_EINVAL;
  *out = nullptr;
  const int rc = check_cfg_b(cfg, n_fits);
  if (rc) return rc;
  if (!dev_workspace || (reinterpret_cast<uintptr_t>(dev_workspace) & 255)) return LSQAMD_EINVAL;
  lsqamdb_fits *f = new (std::nothrow) lsqamdb_fits;
  if (!f) return LSQAMD_ENOMEM;
  f->cfg = *cfg;
  f->B = n_fits;
  f->user_st = reinterpret_cast<hipStream_t>(stream);
  if (carve_b(f, dev_workspace, true) > workspace_bytes) { delete f; return LSQAMD_ENOMEM; }
  carve_b(f, dev_workspace, false);
  // own (capturable) stream: the caller's may be the legacy default stream
  (void)hipGetDevice(&f->dev);
  f->st = lsqamd_host::stream_take();
  if (!f->st) { delete f; return LSQAMD_EHIP; }
  f->opt.xtol = 1e-8; f->opt.gtol = 1e-10; f->opt.ftol = 1e-10;
  f->opt.maxit = 1000; f->opt.scaler = LSQAMD_SCALE_MORE; f->opt.solver = LSQAMD_SOLVER_CHOLESKY;
  f->opt.factor_up = 3.0; f->opt.factor_down = 2.0; f->opt.trs = LSQAMD_TRS_LM; f->opt.avmax = 0.75;
  std::vector<int32_t> wm(4 * (size_t)f->syrk_nwork);
  syrk_work_fill(f->P, f->splits, wm.data());
  if (hipMemcpyAsync(f->syrk_map, wm.data(), wm.size() * sizeof(int32_t), hipMemcpyHostToDevice, f->st) != hipSuccess ||
      hipMemsetAsync(f->M, 0, sizeof(double) * (size_t)(f->B * f->m_stride), f->st) != hipSuccess ||
      hipStreamSynchronize(f->st) != hipSuccess) {
    (void)hipStreamSynchronize(f->st);
    lsqamd_host::stream_give(f->st, f->dev);
    delete f;
    return LSQAMD_EHIP;
  }
  *out = f;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

int lsqamdb_destroy(lsqamdb_fits *f) try {
  if (!f) return 0;
  (void)hipStreamSynchronize(f->st);
  if (f->gexec) (void)hipGraphExecDestroy(f->gexec);
  if (f->graph) (void)hipGraphDestroy(f->graph);
  lsqamd_host::stream_give(f->st, f->dev);       // (synchronised above)
  if (f->jit) lsqamd_jit::release(static_cast<const lsqamd_jit::Kernel *>(f->jit));
  delete f;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

const char *lsqamdb_last_error(const lsqamdb_fits *f) { return f ? f->err.c_str() : "null handle"; }

int lsqamdb_set_x(lsqamdb_fits *f, const double *x, int64_t n_rows, int32_t n_x) try {
  if (!f) return LSQAMD_EINVAL;
  if (!x || n_rows != f->N || n_x != (f->cfg.n_x > 0 ? f->cfg.n_x : 1)) FAIL(f, LSQAMD_EINVAL, "set_x: shape");
  HIPCHK(f, copy_sync(f, f->x, x, sizeof(double) * n_rows * n_x, hipMemcpyHostToDevice));
  f->have_x = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamdb_set_tape(lsqamdb_fits *f, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts) try {
  if (!f) return LSQAMD_EINVAL;
  if (!code || n_code < 1 || n_code > LSQAMD_TAPE_MAX_CODE || n_consts < 0 || n_consts > 1024 || (n_consts > 0 && !consts))
    FAIL(f, LSQAMD_EINVAL, "set_tape: sizes");
  {   // stack discipline and operand ranges (the compiled route indexes by them)
    int sp = 0;
    for (int t = 0; t < n_code; ++t) {
      const int op = code[t] & 0xff, arg = code[t] >> 8;
      bool ok = true;
      if (op == LSQAMD_OP_CONST) { ok = arg >= 0 && arg < n_consts; ++sp; }
      else if (op == LSQAMD_OP_X) { ok = arg >= 0 && arg < (f->cfg.n_x > 0 ? f->cfg.n_x : 1); ++sp; }
      else if (op == LSQAMD_OP_P) { ok = arg >= 0 && arg < f->P; ++sp; }
      else if (op >= LSQAMD_OP_ADD && op <= LSQAMD_OP_POW) { ok = sp >= 2; --sp; }
      else if (op >= LSQAMD_OP_NEG && op <= LSQAMD_OP_LAST) ok = sp >= 1;
      else ok = false;
      if (!ok || sp > LSQAMD_TAPE_MAX_STACK) FAIL(f, LSQAMD_EINVAL, "set_tape: malformed tape at instruction %d", t);
    }
    if (sp != 1) FAIL(f, LSQAMD_EINVAL, "set_tape: the tape must leave exactly one value");
  }
  // the formula compiled (jit.hip): one launch per evaluation with the fits as blockIdx.y, whatever P is -- the
  // interpreter route (forward mode, ceil(P / 16) passes per row) remains for tapes of <= 1024 instructions when
  // hiprtc is absent or the generator declines
  std::string why;
  if (f->jit) lsqamd_jit::release(static_cast<const lsqamd_jit::Kernel *>(f->jit));
  f->jit = lsqamd_jit::compile_tape(code, n_code, consts, n_consts, (int)f->P, f->cfg.n_x > 0 ? f->cfg.n_x : 1, why);
  if (!f->jit && (n_code > 1024 || n_consts > 256))
    FAIL(f, LSQAMD_EUNSUPPORTED, "set_tape: %d instructions need the compiled route, which is unavailable (%s)", n_code, why.c_str());
  if (n_code <= 1024 && n_consts <= 256) {
    HIPCHK(f, copy_sync(f, f->tape, code, sizeof(int32_t) * n_code, hipMemcpyHostToDevice));
    if (n_consts > 0) HIPCHK(f, copy_sync(f, f->consts, consts, sizeof(double) * n_consts, hipMemcpyHostToDevice));
  }
  f->n_tape = n_code;
  f->have_tape = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* shared data: ymean[N], wdiag[N] = 1/sdev of the 1x1 rows */
int lsqamdb_set_data(lsqamdb_fits *f, const double *ymean, const double *wdiag) try {
  if (!f || !ymean || !wdiag) return LSQAMD_EINVAL;
  HIPCHK(f, copy_sync(f, f->ymean, ymean, sizeof(double) * f->N, hipMemcpyHostToDevice));
  HIPCHK(f, copy_sync(f, f->wdiag, wdiag, sizeof(double) * f->N, hipMemcpyHostToDevice));
  f->ymean_stride = 0;
  f->have_data = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* per-fit data means ymean[B*N] (simulated / bootstrap copies of one data set: same
 * covariance, new means); the whitening set by lsqamdb_set_data / _set_blocks is kept */
int lsqamdb_set_data_means(lsqamdb_fits *f, const double *ymean) try {
  if (!f || !ymean) return LSQAMD_EINVAL;
  if (!f->have_data) FAIL(f, LSQAMD_EINVAL, "set_data_means: call lsqamdb_set_data first");
  HIPCHK(f, copy_sync(f, f->ymean, ymean, sizeof(double) * f->B * f->N, hipMemcpyHostToDevice));
  f->ymean_stride = f->N;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* per-fit whitening weights: wdiag[B*N], wt[B*sum_block_sq] (NULL without blocks), DEVICE pointers owned by the caller and
 * valid until the next call or lsqamdb_destroy; tri[n_blocks] replaces the shared flags (0 where ANY fit's block is not
 * triangular).  wdiag = NULL returns to the shared weights of lsqamdb_set_data / _set_blocks. */
int lsqamdb_set_data_weights(lsqamdb_fits *f, const double *wdiag, const double *wt, const int32_t *tri) try {
  if (!f) return LSQAMD_EINVAL;
  (void)hipStreamSynchronize(f->st);
  if (f->gexec) { (void)hipGraphExecDestroy(f->gexec); f->gexec = nullptr; }   // (its nodes hold the old pointers)
  if (f->graph) { (void)hipGraphDestroy(f->graph); f->graph = nullptr; }
  f->ran = false; f->have_cov = false;
  f->pf_wdiag = nullptr; f->pf_wt = nullptr; f->pf_tri.clear();
  if (!wdiag) return 0;
  if (f->cfg.n_blocks > 0 && !tri) FAIL(f, LSQAMD_EINVAL, "set_data_weights: tri is needed with blocks");
  f->pf_wdiag = wdiag; f->pf_wt = wt;
  if (f->cfg.n_blocks > 0) f->pf_tri.assign(tri, tri + f->cfg.n_blocks);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* correlated data blocks shared by all fits; same layout as lsqamd_set_data */
int lsqamdb_set_blocks(lsqamdb_fits *f, int32_t n_blocks, const int64_t *row0, const int64_t *size,
                       const int64_t *modes, const int32_t *tri, const double *wt) try {
  if (!f) return LSQAMD_EINVAL;
  if (n_blocks != f->cfg.n_blocks) FAIL(f, LSQAMD_EINVAL, "set_blocks: n_blocks differs from the config");
  if (n_blocks == 0) { f->have_blocks = true; return 0; }
  if (!row0 || !size || !modes || !tri || !wt) return LSQAMD_EINVAL;
  std::vector<uint8_t> inb((size_t)f->N, 0);
  std::vector<int64_t> woff((size_t)n_blocks);
  f->h_row0.assign(row0, row0 + n_blocks);
  f->h_size.assign(size, size + n_blocks);
  f->h_modes.assign(modes, modes + n_blocks);
  f->h_tri.assign(tri, tri + n_blocks);
  int64_t off = 0;
  for (int32_t k = 0; k < n_blocks; ++k) {
    if (size[k] < 1 || size[k] > f->cfg.max_block || row0[k] < 0 || row0[k] + size[k] > f->N ||
        modes[k] < 0 || modes[k] > size[k])
      FAIL(f, LSQAMD_EINVAL, "set_blocks: block %d out of range", k);
    for (int64_t i = 0; i < size[k]; ++i) {
      if (inb[(size_t)(row0[k] + i)]) FAIL(f, LSQAMD_EINVAL, "set_blocks: blocks overlap");
      inb[(size_t)(row0[k] + i)] = 1;
    }
    woff[(size_t)k] = off;
    off += size[k] * size[k];
  }
  if (off != f->cfg.sum_block_sq) FAIL(f, LSQAMD_EINVAL, "set_blocks: sum of squares differs from the config");
  f->h_woff = woff;
  HIPCHK(f, copy_sync(f, f->in_block, inb.data(), inb.size(), hipMemcpyHostToDevice));
  HIPCHK(f, copy_sync(f, f->blk_row0, row0, sizeof(int64_t) * n_blocks, hipMemcpyHostToDevice));
  HIPCHK(f, copy_sync(f, f->blk_size, size, sizeof(int64_t) * n_blocks, hipMemcpyHostToDevice));
  HIPCHK(f, copy_sync(f, f->blk_woff, woff.data(), sizeof(int64_t) * n_blocks, hipMemcpyHostToDevice));
  HIPCHK(f, copy_sync(f, f->wt, wt, sizeof(double) * off, hipMemcpyDefault));   // host or device source
  f->have_blocks = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* per-fit priors: mean[B*P]; prec[B*P] = 1/sdev^2 per fit (diagonal), or -- cfg.prior_dense -- ONE dense
 * P x P precision shared by all fits (copies of a fit differ in their prior means, not its covariance) */
int lsqamdb_set_priors(lsqamdb_fits *f, const double *mean, const double *prec) try {
  if (!f || !mean || !prec) return LSQAMD_EINVAL;
  if (!f->cfg.has_prior) FAIL(f, LSQAMD_EINVAL, "set_priors: config has no prior");
  HIPCHK(f, copy_sync(f, f->pmean, mean, sizeof(double) * f->B * f->P, hipMemcpyHostToDevice));
  HIPCHK(f, copy_sync(f, f->pprec, prec, sizeof(double) * (f->cfg.prior_dense ? f->P * f->P : f->B * f->P),
                    hipMemcpyDefault));   // host or device source
  f->have_prior = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamdb_set_options(lsqamdb_fits *f, const lsqamd_options *opt) try {
  if (!f || !opt) return LSQAMD_EINVAL;
  if (opt->xtol < 0 || opt->gtol < 0 || opt->maxit < 0 || opt->scaler < 0 || opt->scaler > LSQAMD_SCALE_MARQUARDT)
    FAIL(f, LSQAMD_EINVAL, "set_options: bad value");
  if (opt->trs != LSQAMD_TRS_LM && opt->trs != LSQAMD_TRS_DOGLEG && opt->trs != LSQAMD_TRS_DDOGLEG && opt->trs != LSQAMD_TRS_SUBSPACE2D)
    FAIL(f, LSQAMD_EUNSUPPORTED, "set_options: the batched engine runs alg='lm', 'dogleg', 'ddogleg' and 'subspace2D' only");
  f->opt = *opt;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* run all fits from p0[B*P]; summaries[B] (may be NULL).  use_graph != 0: capture one round in a
 * hipGraph after the first eager round and replay it. */
int lsqamdb_run(lsqamdb_fits *f, const double *p0, lsqamd_summary *summaries, int32_t use_graph) try {
  if (!f || !p0) return LSQAMD_EINVAL;
  int rc = inputs_ready(f);
  if (rc) return rc;
  if (f->timing) use_graph = 0;      // (events around single launches: eager rounds)
  // inputs the caller made on ITS stream (device-resident weights) are complete before the engine's stream reads them.  A null
  // stream is not waited for: synchronising the legacy stream from here would collide with any graph capture another
  // thread has open (see copy_sync); a caller working on the legacy stream orders its own work (include/lsqfit_amd.h)
  if (f->user_st) (void)hipStreamSynchronize(f->user_st);
  RunSpan span{f};
  (void)hipEventRecord(span.e0, f->st);
  if ((rc = start_at(f, p0))) return rc;
  if ((rc = try_one_launch(f, p0)) < 0) return rc;
  if (rc == 0) {   // the lockstep engine
    if ((rc = start_lockstep(f))) return rc;
    int32_t n_active = f->B;
    const int64_t max_rounds = (int64_t)(f->opt.maxit > 0 ? f->opt.maxit : 0) * 17 + 1;
    while (n_active > 0 && f->rounds < max_rounds && f->opt.maxit > 0) {
      if (use_graph && f->rounds >= 1 && !f->gexec) {   // (the first round is eager)
        if ((rc = capture_round(f))) return rc;
        if (!f->gexec) use_graph = 0;
      }
      if (f->gexec) {
        HIPCHK(f, hipGraphLaunch(f->gexec, f->st));
        f->graph_used += 1;
      } else if ((rc = round_any(f))) {
        return rc;
      }
      f->rounds += 1;
      HIPCHK(f, hipMemcpyAsync(&n_active, f->s.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
      HIPCHK(f, hipStreamSynchronize(f->st));
    }
  }
  (void)hipEventRecord(span.e1, f->st);
  (void)hipEventSynchronize(span.e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, span.e0, span.e1);
  f->ran = true;
  f->have_cov = f->one_launch && f->have_cov_from_run;     // (the one-launch kernel leaves covariances and log dets behind)
  return summaries ? write_summaries(f, summaries, ms) : 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamdb_get_x(lsqamdb_fits *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (cap < (size_t)(f->B * f->P)) FAIL(f, LSQAMD_ECAPACITY, "get_x: need %lld", (long long)(f->B * f->P));
  HIPCHK(f, copy_sync(f, out, f->px, sizeof(double) * f->B * f->P, hipMemcpyDeviceToHost));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

/* (J^T J)^-1 of every fit at its final point + log det(J^T J); results stay on the device */
int lsqamdb_covariance(lsqamdb_fits *f, double *logdet_out, size_t cap) try {
  if (!f) return LSQAMD_EINVAL;
  if (!f->ran) FAIL(f, LSQAMD_EINVAL, "covariance: run first");
  const int64_t P = f->P;
  const int32_t B = f->B;
  if (!(f->have_cov && f->one_launch)) {     // (else: formed by the fit kernel itself)
    // the first half of factor_and_solve's chain on its own: P columns instead of ncols_aug, no right-hand side, no mask
    hipLaunchKernelGGL(b_build_damped_kernel, dim3((unsigned)f->ntile, 16, (unsigned)B), dim3(256), 0, f->st, f->red,
                       f->red_stride, P, f->T, f->ldm, f->s.mu, f->diag, (const double *)nullptr, f->red_stride, f->M,
                       f->m_stride, (const int32_t *)nullptr, 0);
    HIPCHK(f, potrf_upper_batched(f->st, f->M, P, f->ldm, P, f->chol_work, f->s.cholinfo, B, f->m_stride, f->w_stride, nullptr));
    hipLaunchKernelGGL(b_logdiag_kernel, dim3((unsigned)B), dim3(256), 0, f->st, f->M, f->m_stride, P, f->ldm, f->logdet);
    HIPCHK(f, trtri_upper_to_lower_T_batched(f->st, f->M, P, f->ldm, f->chol_work, f->Wl, f->ldm, B, f->m_stride, f->w_stride,
                                             f->m_stride));
    GemmTN g;
    g.X = f->Wl; g.Y = f->Wl; g.ldx = g.ldy = f->ldm; g.sx = g.sy = f->m_stride;
    g.C = f->cov; g.ldc = f->ldm; g.sc = f->m_stride;
    g.M = P; g.N = P; g.K = P;
    g.upper_only = 1; g.xy_lower_tri = 1;
    g.batch = B;
    HIPCHK(f, launch_gemm_tn(f->st, g));
    hipLaunchKernelGGL(b_symmetrize_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)P, (unsigned)B), dim3(256), 0,
                       f->st, f->cov, f->m_stride, P, f->ldm);
    HIPCHK(f, hipStreamSynchronize(f->st));
    f->have_cov = true;
  }
  if (logdet_out) {
    if (cap < (size_t)B) FAIL(f, LSQAMD_ECAPACITY, "covariance: need %lld", (long long)B);
    HIPCHK(f, copy_sync(f, logdet_out, f->logdet, sizeof(double) * B, hipMemcpyDeviceToHost));
  }
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamdb_get_cov(lsqamdb_fits *f, int32_t fit, double *out, size_t cap) try {
  if (!f || !out || fit < 0 || fit >= f->B) return LSQAMD_EINVAL;
  const int64_t P = f->P;
  if (cap < (size_t)(P * P)) FAIL(f, LSQAMD_ECAPACITY, "get_cov: need %lld", (long long)(P * P));
  if (!f->have_cov) {
    const int rc = lsqamdb_covariance(f, nullptr, 0);
    if (rc) return rc;
  }
  HIPCHK(f, copy2d_sync(f, out, sizeof(double) * P, f->cov + (int64_t)fit * P * f->ldm, sizeof(double) * f->ldm,
                      sizeof(double) * P, (size_t)P, hipMemcpyDeviceToHost));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamdb_get_cov_all(lsqamdb_fits *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  const int64_t P = f->P, B = f->B;
  if (cap < (size_t)(B * P * P)) FAIL(f, LSQAMD_ECAPACITY, "get_cov_all: need %lld", (long long)(B * P * P));
  if (!f->have_cov) {
    const int rc = lsqamdb_covariance(f, nullptr, 0);
    if (rc) return rc;
  }
  // fit b's rows follow fit b - 1's in f->cov (P rows of ldm doubles each): one strided copy of B * P rows
  HIPCHK(f, copy2d_sync(f, out, sizeof(double) * P, f->cov, sizeof(double) * f->ldm, sizeof(double) * P, (size_t)(B * P),
                      hipMemcpyDeviceToHost));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int32_t lsqamdb_rounds(const lsqamdb_fits *f) { return f ? f->rounds : -1; }

/* the symmetric product of the dogleg family on its own (tests): A[n_fits][P][P] dense, row-major, only its upper triangle read;
 * packs it into the engine's tiles and runs the production kernels.  Scratch is allocated and freed here: not capturable. */
int lsqamdb_op_symv_packed(void *stream, int64_t P, int32_t n_fits, const double *A, const double *u, const int32_t *active,
                           double *y, double *quad) try {
  if (P < 1 || n_fits < 1 || !A || !u || !active || !y || !quad) return LSQAMD_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t npk = packed_doubles(P), npart = symv_packed_partials(P);
  double *scratch = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&scratch), sizeof(double) * (size_t)(n_fits * (npk + npart))) != hipSuccess) {
    (void)hipGetLastError();
    return LSQAMD_ENOMEM;
  }
  double *apk = scratch, *part = scratch + (int64_t)n_fits * npk;
  hipError_t e = launch_pack_dense(st, A, P, P * P, P, n_fits, apk, npk);
  if (e == hipSuccess) e = launch_symv_packed(st, apk, npk, P, n_fits, u, P, part, y, P, quad, 1, active);
  const hipError_t e2 = hipStreamSynchronize(st);
  (void)hipFree(scratch);
  return (e == hipSuccess && e2 == hipSuccess) ? 0 : LSQAMD_EHIP;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

int lsqamdb_timing_enable(lsqamdb_fits *f, int32_t on) try {
  if (!f) return LSQAMD_EINVAL;
  (void)hipStreamSynchronize(f->st);
  f->timing = on != 0;
  give_events(f->tm_syrk, f->dev);
  give_events(f->tm_chol, f->dev);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamdb_timing_get(lsqamdb_fits *f, int32_t which, double *total_ms, int64_t *count) try {
  if (!f || (which != LSQAMD_T_SYRK && which != LSQAMD_T_CHOLESKY)) return LSQAMD_EINVAL;
  (void)hipStreamSynchronize(f->st);
  double tot = 0.0;
  int64_t n = 0;
  for (auto &pr : which == LSQAMD_T_SYRK ? f->tm_syrk : f->tm_chol) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { tot += ms; ++n; }
  }
  if (total_ms) *total_ms = tot;
  if (count) *count = n;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

}  // extern "C"
