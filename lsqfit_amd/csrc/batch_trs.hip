// The dogleg family in the batched engine: dogleg, ddogleg and subspace2D steps for B fits in lockstep.
//
// Per fit these kernels restate what lm_driver.hip does on the host for one fit (legs_preloop, legs_gn, legs_subspace,
// legs_step, the rho / delta rules of iterate), which in turn restates GSL's dogleg.c / subspace2D.c.  What makes the
// family suit lockstep: the two legs of an iterate -- the steepest-descent leg dx_sd = -(|D^-1 g| / |J D^-2 g|)^2 D^-2 g and
// the Gauss-Newton leg dx_gn = -A^-1 g -- depend on (A, g, D) only.  A rejected trial shrinks delta and nothing else, so a
// round in which a fit rejects needs no product and no factorisation for it: the legs are recomputed for the fits that MOVED.
//
// Every step of the family is a combination ca dx_sd + cb dx_gn.  With A dx_gn = -g the quadratic forms of the model reduce to
// three scalars that the legs kernel leaves behind:
//     dx_sd^T A dx_sd = u^4 w^T A w     (u = |D^-1 g| / |J D^-2 g|, w = D^-2 g: ONE symmetric product per iterate)
//     dx_sd^T A dx_gn = -g.dx_sd        dx_gn^T A dx_gn = -g.dx_gn
// so neither the predicted reduction -(dx^T A dx + 2 g.dx) nor subspace2D's 2 x 2 model needs a product per round (the
// single-fit path calls symv_host on dx, d0, d1; the identity holds to the accuracy of the Cholesky solve, i.e. the two paths
// agree to rounding in rho and exactly in the minimum they reach).
//
// The symmetric product reads the packed upper 128 x 128 tiles once (memory bound: 1 MB per fit at P = 512; no MFMA): every
// tile workgroup writes its row contribution and -- off the diagonal -- its transposed contribution as partial vectors,
// a second kernel sums them in a fixed order.  No floating-point atomics: two runs give the same bits.
#include <cmath>

#include "batch.h"

namespace lsqamd {

// ---- y = A u on the packed tiles, stage 1: one workgroup per stored tile and fit ----------------------------------
// tile (tm, tn), tn >= tm:  part[tm][tn][r] = sum_c A[r][c] u[tn 128 + c]        (rows of the tile)
//                           part[tn][tm][c] = sum_r A[r][c] u[tm 128 + r]        (its transpose: the lower triangle's share)
// a diagonal tile contributes its elements on or above the diagonal once each way (the diagonal itself once) and writes
// the sum of both to part[tm][tm].  Every part[k][s] is written by exactly one workgroup.
__global__ __launch_bounds__(256) void b_symv_tiles_kernel(const double *apk, int64_t apk_stride, int64_t P, int64_t T,
                                                           const double *u, int64_t u_stride, double *part,
                                                           const int32_t *active) {
  __shared__ double ur[TBK], uc[TBK], rowp[TBK], colp[4][TBK];
  const int b = blockIdx.y;
  if (!active[b]) return;
  int64_t t = blockIdx.x, tm = 0;
  while (t >= T - tm) { t -= T - tm; ++tm; }
  const int64_t tn = tm + t;
  const bool diag = tm == tn;
  const double *A = apk + b * apk_stride + (int64_t)blockIdx.x * TBK * TBK;
  {
    const int i = threadIdx.x & (TBK - 1);
    const int64_t j = (threadIdx.x < TBK ? tm : tn) * TBK + i;
    const double v = j < P ? u[b * u_stride + j] : 0.0;
    if (threadIdx.x < TBK) ur[i] = v;
    else uc[i] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c0 = lane, c1 = lane + 64;               // a wave reads one 1 KiB row of the tile at a time
  const bool in0 = tn * TBK + c0 < P, in1 = tn * TBK + c1 < P;
  const double u0 = uc[c0], u1 = uc[c1];
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 4
  for (int rr = 0; rr < TBK / 4; ++rr) {
    const int r = rr * 4 + wave;
    const bool rin = tm * TBK + r < P;
    const bool k0 = rin && in0 && (!diag || c0 >= r), k1 = rin && in1 && (!diag || c1 >= r);
    const double a0 = k0 ? A[r * TBK + c0] : 0.0, a1 = k1 ? A[r * TBK + c1] : 0.0;
    const double s = bsum(a0 * u0 + a1 * u1);
    if (lane == 0) rowp[r] = s;
    const double urr = ur[r];
    acc0 += (diag && c0 == r) ? 0.0 : a0 * urr;
    acc1 += (diag && c1 == r) ? 0.0 : a1 * urr;
  }
  colp[wave][c0] = acc0;
  colp[wave][c1] = acc1;
  __syncthreads();
  if (threadIdx.x < TBK) {
    const int i = threadIdx.x;
    const double col = (colp[0][i] + colp[1][i]) + (colp[2][i] + colp[3][i]);
    double *pb = part + (int64_t)b * T * T * TBK;
    if (diag) {
      pb[(tm * T + tm) * TBK + i] = rowp[i] + col;
    } else {
      pb[(tm * T + tn) * TBK + i] = rowp[i];
      pb[(tn * T + tm) * TBK + i] = col;
    }
  }
}

// stage 2: y[j] = sum_s part[j / 128][s][j % 128] in the order of s; quad = u.y ; one workgroup per fit
__global__ __launch_bounds__(256) void b_symv_sum_kernel(const double *part, int64_t P, int64_t T, const double *u,
                                                         int64_t u_stride, double *y, int64_t y_stride, double *quad,
                                                         int64_t q_stride, const int32_t *active) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!active[b]) return;
  const double *pb = part + (int64_t)b * T * T * TBK;
  double q = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const int64_t k = j / TBK, i = j % TBK;
    double a = 0.0;
    for (int64_t s = 0; s < T; ++s) a += pb[(k * T + s) * TBK + i];
    y[b * y_stride + j] = a;
    q += u[b * u_stride + j] * a;
  }
  q = block_sum(q, sh);
  if (threadIdx.x == 0) quad[b * q_stride] = q;
}

__global__ __launch_bounds__(256) void b_pack_dense_kernel(const double *A, int64_t ld, int64_t a_stride, int64_t P,
                                                           int64_t T, double *apk, int64_t apk_stride) {
  const int b = blockIdx.z;
  int64_t t = blockIdx.x, tm = 0;
  while (t >= T - tm) { t -= T - tm; ++tm; }
  const int64_t tn = tm + t;
  double *dst = apk + b * apk_stride + (int64_t)blockIdx.x * TBK * TBK;
  const int c = threadIdx.x & 127;
  for (int rr = (threadIdx.x >> 7); rr < 8; rr += 2) {
    const int r = blockIdx.y * 8 + rr;
    const int64_t i = tm * TBK + r, j = tn * TBK + c;
    dst[r * TBK + c] = (i < P && j < P) ? A[b * a_stride + i * ld + j] : 0.0;
  }
}

// ---- trust_init of the family: delta = 0.3 max(1, |D x0|) (lm_driver.hip do_init) ---------------------------------
__global__ __launch_bounds__(256) void b_trs_init_kernel(int64_t P, const double *diag, const double *x, BTrs t) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  double dxn = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double d = diag[b * P + j], xj = x[b * P + j];
    dxn += d * xj * d * xj;
  }
  dxn = block_sum(dxn, sh);
  if (threadIdx.x == 0) {
    t.rec[b * TR_COUNT + TR_DELTA] = 0.3 * fmax(1.0, sqrt(dxn));
    t.rec[b * TR_COUNT + TR_PRED] = 0.0;
    t.gn_failed[b] = 0;
  }
}

__global__ void b_trs_mask_kernel(int B, BState s, BTrs t) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) t.lmask[b] = (s.moved[b] && s.active[b]) ? 1 : 0;
}

// ---- legs, part 1 (legs_preloop up to the product): w = D^-2 g, |D^-1 g| ------------------------------------------
__global__ __launch_bounds__(256) void b_trs_grad_kernel(int64_t P, const double *gvec, int64_t g_stride, const double *diag,
                                                         BTrs t, const int32_t *mask) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!mask[b]) return;
  double n1 = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double d = diag[b * P + j];
    const double w1 = gvec[b * g_stride + j] / d;
    n1 += w1 * w1;
    t.w[b * P + j] = w1 / d;
  }
  n1 = block_sum(n1, sh);
  if (threadIdx.x == 0) t.rec[b * TR_COUNT + TR_NINVG] = sqrt(n1);
}

// ---- legs, part 2: after w^T A w (launch_symv_packed) and the Gauss-Newton solve at mu = 0 (v = A^-1 g) --------------
// dx_sd, dx_gn, their scaled norms and products with g (legs_preloop, legs_gn); ddogleg's t; the two sums of dogleg_beta;
// subspace2D's c and r (legs_subspace).  A factorisation that failed (cholinfo, non-finite v) is no failed TRIAL: the fit
// stays on the gradient leg (gn_failed), as legs_step does after LSQAMD_ENOTPD.
__global__ __launch_bounds__(256) void b_trs_legs_kernel(int64_t P, int trs, const double *gvec, int64_t g_stride,
                                                         const double *diag, const double *v, int64_t v_stride,
                                                         const int32_t *cholinfo, BTrs t, const int32_t *mask) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  if (!mask[b]) return;
  double *rec = t.rec + b * TR_COUNT;
  const double *g = gvec + b * g_stride, *d = diag + b * P, *w = t.w + b * P, *vb = v + b * v_stride;
  double *sd = t.dx_sd + b * P, *gn = t.dx_gn + b * P;
  const double ninvg = rec[TR_NINVG], waw = rec[TR_WAW];
  const double u = ninvg / sqrt(waw > 0.0 ? waw : 0.0);
  double a_sd = 0.0, a_gsd = 0.0, a_gn = 0.0, a_ggn = 0.0, bad = 0.0;
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    const double s = -(u * u) * w[j];
    sd[j] = s;
    a_sd += d[j] * s * d[j] * s;
    a_gsd += g[j] * s;
    const double vj = vb[j];
    if (!(fabs(vj) < INFINITY)) bad = 1.0;
    gn[j] = -vj;
    a_gn += d[j] * vj * d[j] * vj;
    a_ggn -= g[j] * vj;
  }
  a_sd = block_sum(a_sd, sh);
  a_gsd = block_sum(a_gsd, sh);
  a_gn = block_sum(a_gn, sh);
  a_ggn = block_sum(a_ggn, sh);
  bad = block_sum(bad, sh);
  const bool failed = cholinfo[b] != 0 || bad > 0.0;       // (the same in every thread: block_sum broadcasts)
  const double nsd = sqrt(a_sd), ngn = sqrt(a_gn);
  double tt = 1.0, p0 = 0.0, p1 = 0.0;
  if (!failed && trs == LSQAMD_TRS_DDOGLEG) {
    const double c = u * u * (ninvg / fabs(a_ggn)) * ninvg;
    tt = 1.0 - 0.8 * (1.0 - c);
  }
  if (!failed && trs != LSQAMD_TRS_SUBSPACE2D) {          // dogleg_beta: a, b
    for (int64_t j = threadIdx.x; j < P; j += 256) {
      const double wv = tt * gn[j] - sd[j], d2 = d[j] * d[j];
      p0 += d2 * wv * wv;
      p1 += sd[j] * d2 * wv;
    }
    p0 = block_sum(p0, sh);
    p1 = 2.0 * block_sum(p1, sh);
  } else if (!failed) {                                    // legs_subspace: c = q0.q1, r = |q1 - c q0|
    for (int64_t j = threadIdx.x; j < P; j += 256) p0 += (d[j] * sd[j] / nsd) * (d[j] * gn[j] / ngn);
    p0 = block_sum(p0, sh);
    for (int64_t j = threadIdx.x; j < P; j += 256) {
      const double q = d[j] * gn[j] / ngn - p0 * (d[j] * sd[j] / nsd);
      p1 += q * q;
    }
    p1 = sqrt(block_sum(p1, sh));
  }
  if (threadIdx.x == 0) {
    rec[TR_NSD] = nsd; rec[TR_NGN] = ngn; rec[TR_GSD] = a_gsd; rec[TR_GGN] = a_ggn; rec[TR_T] = tt;
    if (trs == LSQAMD_TRS_SUBSPACE2D) { rec[TR_SC] = p0; rec[TR_SR] = p1; }
    else { rec[TR_BA] = p0; rec[TR_BB] = p1; }
    t.gn_failed[b] = failed ? 1 : 0;
  }
}

// argmin g.q + q.B.q/2 on |q| = delta for a 2 x 2 positive semi-definite B (lm_driver.hip solve_tr_2d; one lane)
__device__ void solve_tr_2d_dev(const double B[2][2], const double g[2], double delta, double q[2]) {
  const double tr = B[0][0] + B[1][1], df = B[0][0] - B[1][1];
  const double rad = sqrt(0.25 * df * df + B[0][1] * B[0][1]);
  const double w0 = 0.5 * tr - rad, w1 = 0.5 * tr + rad;
  double v0[2], v1[2];
  if (fabs(B[0][1]) > 0.0) {
    v1[0] = w1 - B[1][1]; v1[1] = B[0][1];
    const double n = hypot(v1[0], v1[1]);
    v1[0] /= n; v1[1] /= n;
  } else if (B[0][0] >= B[1][1]) { v1[0] = 1.0; v1[1] = 0.0; }
  else { v1[0] = 0.0; v1[1] = 1.0; }
  v0[0] = -v1[1]; v0[1] = v1[0];
  const double g0 = v0[0] * g[0] + v0[1] * g[1], g1 = v1[0] * g[0] + v1[1] * g[1];
  double lo = 0.0, hi = fmax(1.0, hypot(g[0], g[1]) / delta);
  // (bounded: a double cannot be doubled more than 2098 times before it is infinite, where |q| = 0)
  for (int k = 0; k < 2100 && hypot(g0 / (w0 + hi), g1 / (w1 + hi)) > delta; ++k) hi *= 2.0;
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (hypot(g0 / (w0 + mid), g1 / (w1 + mid)) > delta) lo = mid;
    else hi = mid;
    if (hi - lo <= 1e-16 * hi) break;
  }
  const double lam = 0.5 * (lo + hi);
  const double c0 = -g0 / (w0 + lam), c1 = -g1 / (w1 + lam);
  q[0] = v0[0] * c0 + v1[0] * c1;
  q[1] = v0[1] * c0 + v1[1] * c1;
}

// ---- the trial step for the current delta (legs_step): dx = ca dx_sd + cb dx_gn, x_trial, predicted reduction ------------
__global__ __launch_bounds__(256) void b_trs_step_kernel(int64_t P, int trs, const double *x, double *xt, double *dx, BTrs t,
                                                         const int32_t *active) {
  __shared__ double coef[2];
  const int b = blockIdx.x;
  if (!active[b]) return;
  double *rec = t.rec + b * TR_COUNT;
  if (threadIdx.x == 0) {
    const double delta = rec[TR_DELTA], nsd = rec[TR_NSD], ngn = rec[TR_NGN], gsd = rec[TR_GSD], ggn = rec[TR_GGN];
    const bool failed = t.gn_failed[b] != 0;
    double ca = 0.0, cb = 0.0;                    // (a zero coefficient: that leg is not read at all)
    if (trs == LSQAMD_TRS_SUBSPACE2D) {
      const double c = rec[TR_SC], r = rec[TR_SR];
      if (failed) ca = delta / nsd;
      else if (ngn <= delta) cb = 1.0;
      else if (!(r > 20.0 * (double)(P + 2) * 2.220446049250313e-16)) ca = delta / nsd;   // gsl_linalg_QRPT_rank's tolerance
      else {
        // the model in the basis d0 = dx_sd / nsd, d1 = (dx_gn / ngn - c d0) / r, from the three forms above
        const double u = rec[TR_NINVG] / sqrt(rec[TR_WAW] > 0.0 ? rec[TR_WAW] : 0.0);
        const double S = u * u * u * u * rec[TR_WAW] / (nsd * nsd), M = -gsd / (nsd * ngn), G = -ggn / (ngn * ngn);
        double Bm[2][2], gm[2], q[2];
        Bm[0][0] = S;
        Bm[0][1] = Bm[1][0] = (M - c * S) / r;
        Bm[1][1] = (G - 2.0 * c * M + c * c * S) / (r * r);
        gm[0] = gsd / nsd;
        gm[1] = (ggn / ngn - c * gsd / nsd) / r;
        solve_tr_2d_dev(Bm, gm, delta, q);
        ca = (q[0] - q[1] * c / r) / nsd;
        cb = q[1] / (r * ngn);
      }
    } else {
      if (nsd >= delta) ca = delta / nsd;
      else if (failed) ca = 1.0;
      else if (ngn <= delta) cb = 1.0;
      else {
        const double tt = rec[TR_T];
        if (trs == LSQAMD_TRS_DDOGLEG && tt * ngn <= delta) cb = delta / ngn;
        else {
          const double a = rec[TR_BA], bq = rec[TR_BB];
          const double c = (nsd + delta) * (nsd - delta);
          const double disc = sqrt(bq * bq - 4.0 * a * c);
          const double beta = bq > 0.0 ? (-2.0 * c) / (bq + disc) : (-bq + disc) / (2.0 * a);
          ca = 1.0 - beta;
          cb = beta * tt;
        }
      }
    }
    coef[0] = ca; coef[1] = cb;
    // -(dx^T A dx + 2 g.dx) with dx_sd^T A dx_sd = u^4 w^T A w, dx_sd^T A dx_gn = -g.dx_sd, dx_gn^T A dx_gn = -g.dx_gn
    const double u = rec[TR_NINVG] / sqrt(rec[TR_WAW] > 0.0 ? rec[TR_WAW] : 0.0);
    double quad = 0.0, lin = 0.0;
    if (ca != 0.0) { quad += ca * ca * (u * u * u * u * rec[TR_WAW]); lin += ca * gsd; }
    if (cb != 0.0) { quad += -cb * cb * ggn; lin += cb * ggn; }
    if (ca != 0.0 && cb != 0.0) quad += -2.0 * ca * cb * gsd;
    rec[TR_PRED] = -(quad + 2.0 * lin);
  }
  __syncthreads();
  const double ca = coef[0], cb = coef[1];
  for (int64_t j = threadIdx.x; j < P; j += 256) {
    double s = 0.0;
    if (ca != 0.0) s = ca * t.dx_sd[b * P + j];
    if (cb != 0.0) s += cb * t.dx_gn[b * P + j];
    dx[b * P + j] = s;
    xt[b * P + j] = x[b * P + j] + s;
  }
}

// ---- rho, delta, accept / reject (lm_driver.hip iterate, after the trial's chi2); one thread per fit ---------------------
__global__ void b_trs_decide_kernel(int B, double factor_up, double factor_down, BState s, BTrs t) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  s.moved[b] = 0;
  if (!s.active[b]) return;
  double rho = -1.0;
  const double normf = sqrt(s.chi2[b]), normf_t = sqrt(s.chi2t[b]);
  if (normf_t < normf) {   // NaN-safe: anything else rejects
    const double u = normf_t / normf;
    const double actual = 1.0 - u * u;
    const double pred = t.rec[b * TR_COUNT + TR_PRED] / s.chi2[b];
    rho = pred > 0.0 ? actual / pred : -1.0;
  }
  if (rho > 0.75) t.rec[b * TR_COUNT + TR_DELTA] *= factor_up;
  else if (rho < 0.25) t.rec[b * TR_COUNT + TR_DELTA] /= factor_down;
  s.accepted[b] = 0;
  s.enoprog[b] = 0;
  if (rho > 0.0) {
    s.accepted[b] = 1;
    s.moved[b] = 1;
    s.bad[b] = 0;
  } else {
    s.bad[b] += 1;
    if (s.bad[b] > 15) {
      s.enoprog[b] = 1;
      s.bad[b] = 0;
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
hipError_t launch_symv_packed(hipStream_t st, const double *apk, int64_t apk_stride, int64_t P, int32_t B, const double *u,
                              int64_t u_stride, double *part, double *y, int64_t y_stride, double *quad, int64_t q_stride,
                              const int32_t *active) {
  const int64_t T = (P + TBK - 1) / TBK;
  hipLaunchKernelGGL(b_symv_tiles_kernel, dim3((unsigned)(T * (T + 1) / 2), (unsigned)B), dim3(256), 0, st, apk, apk_stride, P, T,
                     u, u_stride, part, active);
  hipLaunchKernelGGL(b_symv_sum_kernel, dim3((unsigned)B), dim3(256), 0, st, part, P, T, u, u_stride, y, y_stride, quad,
                     q_stride, active);
  return hipGetLastError();
}

hipError_t launch_pack_dense(hipStream_t st, const double *A, int64_t ld, int64_t a_stride, int64_t P, int32_t B, double *apk,
                             int64_t apk_stride) {
  const int64_t T = (P + TBK - 1) / TBK;
  hipLaunchKernelGGL(b_pack_dense_kernel, dim3((unsigned)(T * (T + 1) / 2), 16, (unsigned)B), dim3(256), 0, st, A, ld, a_stride, P,
                     T, apk, apk_stride);
  return hipGetLastError();
}

hipError_t launch_trs_init(hipStream_t st, int64_t P, int32_t B, const double *diag, const double *x, BTrs t) {
  hipLaunchKernelGGL(b_trs_init_kernel, dim3((unsigned)B), dim3(256), 0, st, P, diag, x, t);
  return hipGetLastError();
}

hipError_t launch_trs_mask(hipStream_t st, int32_t B, BState s, BTrs t) {
  hipLaunchKernelGGL(b_trs_mask_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (int)B, s, t);
  return hipGetLastError();
}

hipError_t launch_trs_grad(hipStream_t st, int64_t P, int32_t B, const double *gvec, int64_t g_stride, const double *diag, BTrs t,
                           const int32_t *mask) {
  hipLaunchKernelGGL(b_trs_grad_kernel, dim3((unsigned)B), dim3(256), 0, st, P, gvec, g_stride, diag, t, mask);
  return hipGetLastError();
}

hipError_t launch_trs_legs(hipStream_t st, int64_t P, int32_t B, int trs, const double *gvec, int64_t g_stride, const double *diag,
                           const double *v, int64_t v_stride, const int32_t *cholinfo, BTrs t, const int32_t *mask) {
  hipLaunchKernelGGL(b_trs_legs_kernel, dim3((unsigned)B), dim3(256), 0, st, P, trs, gvec, g_stride, diag, v, v_stride, cholinfo, t,
                     mask);
  return hipGetLastError();
}

hipError_t launch_trs_step(hipStream_t st, int64_t P, int32_t B, int trs, const double *x, double *xt, double *dx, BTrs t,
                           const int32_t *active) {
  hipLaunchKernelGGL(b_trs_step_kernel, dim3((unsigned)B), dim3(256), 0, st, P, trs, x, xt, dx, t, active);
  return hipGetLastError();
}

hipError_t launch_trs_decide(hipStream_t st, int32_t B, double factor_up, double factor_down, BState s, BTrs t) {
  hipLaunchKernelGGL(b_trs_decide_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (int)B, factor_up, factor_down, s, t);
  return hipGetLastError();
}

}  // namespace lsqamd
