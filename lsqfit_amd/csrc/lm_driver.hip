// The host side of the trust-region drivers (gfx950 build, host code only).
//
// They restate GSL's multifit_nlinear trust/lm/nielsen/scaling/convergence logic that src/lsqfit/_gsl.pyx:676-677 runs
// (init + driver), on the normal equations (solver='cholesky').  All O(N P), O(N P^2) and O(P^3) work is on the device
// (eval.hip); the host keeps only O(P) vectors (x, g, D, dx) and the scalars (mu, nu, rho), so that every rank of a
// row-sharded fit takes identical decisions from the identical all-reduced (J^T J, J^T f, chi2).  Nothing is uploaded
// inside a step (D and the trial point are mirrored / formed on the device); one stream synchronisation per trial step
// and one per Jacobian.  Here: what every host-driven method does with a trial point (upload_point, trial_residual,
// accept_trial; scipy_methods.hip uses them too), the start of a fit (do_init), one trust_iterate for every method (iterate:
// a step proposed -- propose_lm, propose_legs -- then evaluated and accepted or rejected, for lm, lmaccel, dogleg, ddogleg,
// subspace2D on the host; iterate_device: plain lm with its state on the device, its half steps replayed from captured graphs,
// their records polled from pinned memory; iterate_varpro: linear parameters projected out), the convergence test, the driver
// loop (driver_iteration, run_gsl_driver), the summary, and the whole small fit in one launch (run_one_launch).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <string>
#include <vector>
#include <sched.h>

#include "host.h"

using namespace lsqamd;

namespace lsqamd_host {

// spin-wait hint of the host polling loops
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#else
  sched_yield();
#endif
}

// Wait for a record a kernel publishes into pinned memory: spin on arrived() (the clock is looked at every 64 spins), yield
// the core between looks once 200 us have passed (a long half step: stop hogging it), give up after budget_us.
// -> whether it arrived; what to do when it did not (the stream, then the device's own copy) is the caller's business
template <typename Arrived>
static bool poll(Arrived &&arrived, int budget_us) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    if (arrived()) return true;
    cpu_relax();
    if ((spins & 63) == 0) {
      const auto dt = std::chrono::steady_clock::now() - t0;
      if (dt > std::chrono::microseconds(budget_us)) return false;
      if (dt > std::chrono::microseconds(200)) sched_yield();
    }
  }
}

struct Legs {  // dogleg.c / subspace2D.c state for one trust_iterate
  std::vector<double> dx_sd, dx_gn, q0, q1;
  double norm_Dsd = 0.0, norm_Dgn = -1.0, norm_Dinvg = 0.0, norm_JDinv2g = 0.0;
  bool gn_failed = false;
  int sub = -1;  // subspace2D basis: -1 not built, 0 legs parallel, 1 ready
  double subg[2] = {0, 0}, subB[2][2] = {{0, 0}, {0, 0}};
};

double scaled_norm(const std::vector<double> &d, const std::vector<double> &v) {
  double s = 0.0;
  for (size_t i = 0; i < v.size(); ++i) s += d[i] * v[i] * d[i] * v[i];
  return std::sqrt(s);
}

// dogleg_preloop: steepest-descent leg dx_sd = -alpha D^-2 g, alpha = |D^-1 g|^2 / |J D^-2 g|^2
int legs_preloop(lsqamd_fit *f, Legs &L) {
  const int64_t P = f->P;
  std::vector<double> w2(P), Aw(P);
  double n1 = 0.0;
  for (int64_t j = 0; j < P; ++j) {
    const double w1 = f->hg[j] / f->hdiag[j];
    n1 += w1 * w1;
    w2[j] = w1 / f->hdiag[j];
  }
  L.norm_Dinvg = std::sqrt(n1);
  int rc = symv_host(f, w2.data(), Aw.data());
  if (rc) return rc;
  const double q = dot_h(w2, Aw);
  L.norm_JDinv2g = std::sqrt(q > 0.0 ? q : 0.0);
  const double u = L.norm_Dinvg / L.norm_JDinv2g;
  L.dx_sd.resize(P);
  for (int64_t j = 0; j < P; ++j) L.dx_sd[j] = -(u * u) * w2[j];
  L.norm_Dsd = scaled_norm(f->hdiag, L.dx_sd);
  L.norm_Dgn = -1.0;
  L.gn_failed = false;
  L.sub = -1;
  return 0;
}

// Gauss-Newton leg: the damped solve at mu = 0 (dogleg_calc_gn)
int legs_gn(lsqamd_fit *f, Legs &L) {
  if (L.norm_Dgn >= 0.0 || L.gn_failed) return 0;
  const int rc = solve_damped_dev(f, 0.0, f->hdiag.data());
  if (rc < 0 && rc != LSQAMD_ENOTPD) return rc;
  if (rc == LSQAMD_ENOTPD) {  // singular J^T J: no Gauss-Newton point, stay on the gradient leg
    L.gn_failed = true;
    return 0;
  }
  L.dx_gn.resize(f->P);
  for (int64_t j = 0; j < f->P; ++j) L.dx_gn[j] = -f->hv[j];
  L.norm_Dgn = scaled_norm(f->hdiag, L.dx_gn);
  return 0;
}

double dogleg_beta(const lsqamd_fit *f, const Legs &L, double t, double delta) {
  double a = 0.0, b = 0.0;
  for (int64_t j = 0; j < f->P; ++j) {
    const double w = t * L.dx_gn[j] - L.dx_sd[j];
    const double d2 = f->hdiag[j] * f->hdiag[j];
    a += d2 * w * w;
    b += L.dx_sd[j] * d2 * w;
  }
  b *= 2.0;
  const double c = (L.norm_Dsd + delta) * (L.norm_Dsd - delta);
  const double disc = std::sqrt(b * b - 4.0 * a * c);
  return b > 0.0 ? (-2.0 * c) / (b + disc) : (-b + disc) / (2.0 * a);
}

// argmin g.q + q.B.q/2 on |q| = delta for a 2 x 2 positive semi-definite B (secular equation)
void solve_tr_2d(const double B[2][2], const double g[2], double delta, double q[2]) {
  const double tr = B[0][0] + B[1][1], df = B[0][0] - B[1][1];
  const double rad = std::sqrt(0.25 * df * df + B[0][1] * B[0][1]);
  const double w0 = 0.5 * tr - rad, w1 = 0.5 * tr + rad;
  double v0[2], v1[2];  // eigenvectors
  if (std::fabs(B[0][1]) > 0.0) {
    v1[0] = w1 - B[1][1]; v1[1] = B[0][1];
    const double n = std::hypot(v1[0], v1[1]);
    v1[0] /= n; v1[1] /= n;
  } else if (B[0][0] >= B[1][1]) { v1[0] = 1.0; v1[1] = 0.0; }
  else { v1[0] = 0.0; v1[1] = 1.0; }
  v0[0] = -v1[1]; v0[1] = v1[0];
  const double g0 = v0[0] * g[0] + v0[1] * g[1], g1 = v1[0] * g[0] + v1[1] * g[1];
  auto qnorm = [&](double lam) { return std::hypot(g0 / (w0 + lam), g1 / (w1 + lam)); };
  double lo = 0.0, hi = std::fmax(1.0, std::hypot(g[0], g[1]) / delta);
  while (qnorm(hi) > delta) hi *= 2.0;
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (qnorm(mid) > delta) lo = mid; else hi = mid;
    if (hi - lo <= 1e-16 * hi) break;
  }
  const double lam = 0.5 * (lo + hi);
  const double c0 = -g0 / (w0 + lam), c1 = -g1 / (w1 + lam);
  q[0] = v0[0] * c0 + v1[0] * c1;
  q[1] = v0[1] * c0 + v1[1] * c1;
}

// orthonormal basis of span(D dx_sd, D dx_gn) and the 2 x 2 model in it (subspace2D_preloop)
int legs_subspace(lsqamd_fit *f, Legs &L) {
  if (L.sub >= 0) return 0;
  const int64_t P = f->P;
  L.q0.resize(P); L.q1.resize(P);
  double c = 0.0;
  for (int64_t j = 0; j < P; ++j) {
    L.q0[j] = f->hdiag[j] * L.dx_sd[j] / L.norm_Dsd;
    L.q1[j] = f->hdiag[j] * L.dx_gn[j] / L.norm_Dgn;
    c += L.q0[j] * L.q1[j];
  }
  double r = 0.0;
  for (int64_t j = 0; j < P; ++j) { L.q1[j] -= c * L.q0[j]; r += L.q1[j] * L.q1[j]; }
  r = std::sqrt(r);
  if (!(r > 20.0 * (double)(P + 2) * DBL_EPS)) {  // gsl_linalg_QRPT_rank default tolerance
    L.sub = 0;
    return 0;
  }
  for (int64_t j = 0; j < P; ++j) L.q1[j] /= r;
  std::vector<double> d0(P), d1(P), A0(P), A1(P);
  for (int64_t j = 0; j < P; ++j) { d0[j] = L.q0[j] / f->hdiag[j]; d1[j] = L.q1[j] / f->hdiag[j]; }
  int rc = symv_host(f, d0.data(), A0.data());
  if (rc) return rc;
  rc = symv_host(f, d1.data(), A1.data());
  if (rc) return rc;
  L.subB[0][0] = dot_h(d0, A0); L.subB[0][1] = L.subB[1][0] = dot_h(d0, A1); L.subB[1][1] = dot_h(d1, A1);
  L.subg[0] = dot_h(d0, f->hg); L.subg[1] = dot_h(d1, f->hg);
  L.sub = 1;
  return 0;
}

// trs->step for the dogleg family: dx for the current trust radius
int legs_step(lsqamd_fit *f, Legs &L, std::vector<double> &dx) {
  const int64_t P = f->P;
  const double delta = f->delta;
  const int trs = f->opt.trs;
  auto scaled = [&](const std::vector<double> &v, double s) { for (int64_t j = 0; j < P; ++j) dx[j] = s * v[j]; };
  if (trs == LSQAMD_TRS_SUBSPACE2D) {
    int rc = legs_gn(f, L);
    if (rc) return rc;
    if (L.gn_failed) { scaled(L.dx_sd, delta / L.norm_Dsd); return 0; }
    if (L.norm_Dgn <= delta) { dx = L.dx_gn; return 0; }
    rc = legs_subspace(f, L);
    if (rc) return rc;
    if (L.sub == 0) { scaled(L.dx_sd, delta / L.norm_Dsd); return 0; }
    double q[2];
    solve_tr_2d(L.subB, L.subg, delta, q);
    for (int64_t j = 0; j < P; ++j) dx[j] = (L.q0[j] * q[0] + L.q1[j] * q[1]) / f->hdiag[j];
    return 0;
  }
  if (L.norm_Dsd >= delta) { scaled(L.dx_sd, delta / L.norm_Dsd); return 0; }
  int rc = legs_gn(f, L);
  if (rc) return rc;
  if (L.gn_failed) { dx = L.dx_sd; return 0; }
  if (L.norm_Dgn <= delta) { dx = L.dx_gn; return 0; }
  double t = 1.0;
  if (trs == LSQAMD_TRS_DDOGLEG) {
    const double u = L.norm_Dinvg / L.norm_JDinv2g;
    const double gd = dot_h(f->hg, L.dx_gn);
    const double c = u * u * (L.norm_Dinvg / std::fabs(gd)) * L.norm_Dinvg;
    t = 1.0 - 0.8 * (1.0 - c);
    if (t * L.norm_Dgn <= delta) { scaled(L.dx_gn, delta / L.norm_Dgn); return 0; }
  }
  const double beta = dogleg_beta(f, L, t, delta);
  for (int64_t j = 0; j < P; ++j) dx[j] = L.dx_sd[j] + beta * (t * L.dx_gn[j] - L.dx_sd[j]);
  return 0;
}

// ---- what every host-driven method does with a trial point (declared in fit_state.h: scipy_methods.hip too) ----
// x_host -> the device vector dst_dev (p_trial; p_dev for a start) through the pinned staging vector.  Queued only
int upload_point(lsqamd_fit *f, double *dst_dev, const double *x_host) {
  std::memcpy(f->pin_x, x_host, sizeof(double) * f->P);
  HIPCHK(f, hipMemcpyAsync(dst_dev, f->pin_x, sizeof(double) * f->P, hipMemcpyHostToDevice, f->st));
  return 0;
}

// x_host becomes the trial point (p_trial); chi2 there.  Counts one nfev
int trial_residual(lsqamd_fit *f, const double *x_host, double *chi2) {
  const int rc = upload_point(f, f->p_trial, x_host);
  return rc ? rc : eval_residual_dev(f, f->p_trial, chi2);
}

// The trial point (x_new on the host, p_trial on the device) becomes the current one: J, A, g, chi2 there (one njev), the
// buffers swapped, D updated where the method rescales.  hdx stays with the caller: its sign and timing differ per method
int accept_trial(lsqamd_fit *f, const std::vector<double> &x_new, bool rescale) {
  const int rc = eval_normal_dev(f, f->p_trial);
  if (rc) return rc;
  f->hx = x_new;
  std::swap(f->p_dev, f->p_trial);
  if (rescale) scale_update(f);
  return 0;
}

// trust_eval_step's rho: actual over predicted reduction, pred_num = the predicted one times chi2_cur.  -1 rejects
// (NaN-safe: anything but a smaller |f| does)
static double gain_ratio(double chi2_cur, double chi2_trial, double pred_num) {
  const double normf = std::sqrt(chi2_cur), normf_t = std::sqrt(chi2_trial);
  if (!(normf_t < normf)) return -1.0;
  const double u = normf_t / normf;
  const double pred = pred_num / chi2_cur;
  return pred > 0.0 ? (1.0 - u * u) / pred : -1.0;
}

// nielsen.c: the damping after an accepted and after a rejected trial
static void nielsen_accept(lsqamd_fit *f, double rho) {
  const double b = 2.0 * rho - 1.0;
  f->mu *= std::fmax(0.333333333333333, 1.0 - b * b * b);
  f->nu = 2;
}
static void nielsen_reject(lsqamd_fit *f) {
  f->mu *= (double)f->nu;
  f->nu <<= 1;
}

// ---- variable projection (nonlinear_fit's linear=, src/lsqfit/__init__.py:738-787) -------------
// The residual is linear in the masked parameters a, and the reference hands the plugin
// phi(theta) = min_a chi2(a, theta): its wrapped fit function solves for a at EVERY evaluation.
// Here: every trial point gets a full evaluation (A_t, g_t, chi2_t) followed by the exact linear
// solve A_aa da = -g_a (the masked build of the damped matrix, theta frozen) and
// chi2(a + da, theta_t) = chi2_t + g_a.da; the step in theta is the LM step of the projected
// functional, (S + mu D_t^2) dtheta = -g_t with the Schur complement S = A_tt - A_ta A_aa^-1 A_at,
// obtained by solving the full system with the a-block of the damping matrix set to zero
// (Kaufman's form of the Golub-Pereyra Jacobian; the reference differentiates through its lstsq
// and keeps the second term too: same minimum, slightly different iterates).  An accepted point
// is evaluated once more at the projected a; a rejected trial restores (A, g) from a device copy.
struct VarproStash {   // the current point's (A | g | chi2) block and host mirrors while a trial's evaluation overwrites them
  int64_t n = 0;             // doubles of redbuf
  bool on_device = true;     // kept in f->cov; tiny P (the tile padding exceeds P x ldm): on the host
  std::vector<double> host, g, coln;
  double chi2 = 0.0;
};
static int varpro_stash(lsqamd_fit *f, VarproStash &k) {
  k.g = f->hg; k.coln = f->hcoln;
  k.chi2 = f->chi2;
  if (k.on_device) {
    HIPCHK(f, hipMemcpyAsync(f->cov, f->redbuf, sizeof(double) * k.n, hipMemcpyDeviceToDevice, f->st));
  } else {
    k.host.resize(k.n);
    HIPCHK(f, hipMemcpyAsync(k.host.data(), f->redbuf, sizeof(double) * k.n, hipMemcpyDeviceToHost, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
  }
  return 0;
}
static int varpro_restore(lsqamd_fit *f, const VarproStash &k) {   // back to the current point's A, g
  if (k.on_device) HIPCHK(f, hipMemcpyAsync(f->redbuf, f->cov, sizeof(double) * k.n, hipMemcpyDeviceToDevice, f->st));
  else {   // (on the handle's stream: the library never touches the legacy default stream -- see copy_sync in batch.hip)
    HIPCHK(f, hipMemcpyAsync(f->redbuf, k.host.data(), sizeof(double) * k.n, hipMemcpyHostToDevice, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
  }
  f->hg = k.g; f->hcoln = k.coln;
  f->chi2 = k.chi2;
  f->have_dense_A = false;
  return 0;
}

// One trial of the projected functional, from the damped step in f->hv (dt: the damping it was solved with): the current
// point's (A, g) stashed, the full evaluation at x - v, the exact linear solve there.  -> xt, the trial point with its linear
// parameters projected; hdx; *rho, its gain ratio (left alone when the trial point has no finite chi2 or no linear solve)
static int varpro_trial(lsqamd_fit *f, const std::vector<double> &dt, const std::vector<double> &frozen, VarproStash &keep,
                        std::vector<double> &xt, double *rho) {
  const int64_t P = f->P;
  const double chi2_cur = f->chi2;
  double vg = 0.0, dv2 = 0.0;
  for (int64_t j = 0; j < P; ++j) {
    const double v = f->hv[j];
    vg += v * f->hg[j];
    dv2 += dt[j] * v * dt[j] * v;
    xt[j] = f->hx[j] - v;
  }
  const double pred_num = vg + f->mu * dv2;      // |J v|^2 + 2 mu |D v|^2 by the system v solves
  int rc = varpro_stash(f, keep);
  if (rc || (rc = upload_point(f, f->p_trial, xt.data()))) return rc;
  rc = eval_normal_dev(f, f->p_trial);           // full evaluation at the trial point ...
  f->nfev++;
  if (rc < 0 && rc != LSQAMD_ENONFINITE) return rc;
  if (rc == 0) {
    rc = solve_damped_dev(f, 0.0, nullptr, frozen.data());   // ... and the exact linear solve there
    if (rc < 0 && rc != LSQAMD_ENOTPD) return rc;
  }
  if (rc != 0) return 0;
  double chi2_t = f->chi2;
  for (int64_t j = 0; j < P; ++j)
    if (f->linear[j]) { chi2_t -= f->hg[j] * f->hv[j]; xt[j] -= f->hv[j]; }
  for (int64_t j = 0; j < P; ++j) f->hdx[j] = xt[j] - f->hx[j];   // trial steps count for the xtol test
  *rho = gain_ratio(chi2_cur, chi2_t > 0.0 ? chi2_t : 0.0, pred_num);
  return 0;
}

int iterate_varpro(lsqamd_fit *f) {
  const int64_t P = f->P;
  VarproStash keep;
  keep.n = f->npk + P + 1;
  keep.on_device = P * f->ldm >= keep.n;
  std::vector<double> dt(P), frozen(P), xt(P);
  for (int64_t j = 0; j < P; ++j) frozen[j] = f->linear[j] ? 0.0 : 1.0;
  int bad_steps = 0;
  while (true) {
    for (int64_t j = 0; j < P; ++j) dt[j] = f->linear[j] ? 0.0 : f->hdiag[j];
    double rho = -1.0;
    int rc = solve_damped_dev(f, f->mu, dt.data());
    if (rc < 0 && rc != LSQAMD_ENOTPD) return rc;
    const bool tried = rc == 0;
    if (tried && (rc = varpro_trial(f, dt, frozen, keep, xt, &rho))) return rc;
    if (rho > 0.0) {
      // the point with its linear parameters projected is not the one the trial evaluated: J, A, g there, one more nfev
      if ((rc = upload_point(f, f->p_trial, xt.data()))) return rc;
      f->nfev++;
      if ((rc = accept_trial(f, xt, true))) return rc;
      nielsen_accept(f, rho);
      return 0;
    }
    if (tried && (rc = varpro_restore(f, keep))) return rc;
    nielsen_reject(f);
    if (++bad_steps > 15) {
      rc = eval_normal_dev(f, f->p_dev);  // leave J, f of the CURRENT point behind
      return rc ? rc : LSQAMD_ENOPROG;
    }
  }
}

// One trust_iterate of plain lm with the state on the device: per trial the host queues
//   solve -> (trial point, v.g, |D v|^2) -> residual (+ all-reduce) -> decision (rho, mu, nu, delta)
// and reads ONE 128-byte record; an accepted trial queues the Jacobian, the normal equations, the
// update of D and the convergence test and reads the record once more.  No P-length vector
// crosses PCIe, no P-length loop runs on the host.
// The two halves of a device-resident LM step as launch sequences (no host reads in between), so that
// each can be captured once per p-buffer parity and replayed: small problems spend more host time
// launching their ~35 kernels than the GPU spends running them.

// the LM record from the device into pin_lm, behind what has been queued
static int fetch_record(lsqamd_fit *f) {
  HIPCHK(f, hipMemcpyAsync(f->pin_lm, f->lmd, sizeof(double) * LMS_COUNT, hipMemcpyDeviceToHost, f->st));
  return 0;
}
// ... at the end of a half step, unless its kernels mirror the record into pin_lm themselves (zero copy)
static int publish_record(lsqamd_fit *f) { return f->lm_zero_copy ? 0 : fetch_record(f); }

static int enqueue_trial(lsqamd_fit *f) {
  const int64_t P = f->P;
  double *gvec = f->redbuf + f->npk;
  const bool watch = f->opt.solver == LSQAMD_SOLVER_QR;    // solver = qr: how much of each column its pivot retained
  if (small_fuse(f) && P <= 32) {
    // up to 32 parameters: the whole trial solve (build, factor, substitute, trial point, record) by one wave
    // out of the packed tile -- one launch instead of six
    {
      Scope sc(f, LSQAMD_T_CHOLESKY);
      if (P <= 12)
        HIPCHK(f, launch_lm_tiny12_solve(f->st, f->redbuf, P, gvec, f->dscale, f->p_dev, f->p_trial, f->yv + P, f->lmd, f->info_dev,
                                         watch ? 1 : 0));
      else
        HIPCHK(f, launch_lm_small_solve(f->st, f->redbuf, P, gvec, f->dscale, f->p_dev, f->p_trial, f->yv + P, f->lmd, f->info_dev,
                                        watch ? 1 : 0));
    }
    const int rct = eval_residual_launch(f, f->p_trial, true);
    if (rct) return rct;
    return publish_record(f);
  }
  const bool small = small_fuse(f) && (P == 128 || P == 256);   // (whole 128-blocks: the kernel's GEMVs read full tiles)
  int rc = solve_damped_launch(f, f->mu, nullptr, nullptr, false, f->lmd + LMS_MU, small);
  if (rc) return rc;
  if (small) {
    Scope sc(f, LSQAMD_T_SOLVE);
    HIPCHK(f, launch_lm_solve_tail_small(f->st, f->M, f->ldm, P, f->chol_work, f->p_dev, gvec, f->dscale, f->p_trial, f->yv + P,
                                         f->lmd, watch ? f->diag_dev : nullptr, f->info_dev));
  } else {
    HIPCHK(f, launch_lm_trial(f->st, P, f->p_dev, f->yv + P, gvec, f->dscale, f->p_trial, f->lmd, watch ? f->M : nullptr, f->ldm,
                              watch ? f->diag_dev : nullptr));
  }
  const bool alone = !f->comm && !f->reduce;
  rc = eval_residual_launch(f, f->p_trial, alone);
  if (rc) return rc;
  if (!alone)
    HIPCHK(f, launch_lm_decide(f->st, f->red_scalar, f->info_dev, f->opt.factor_up, f->opt.factor_down, f->lmd));
  return publish_record(f);
}

static int enqueue_accept(lsqamd_fit *f) {   // p_trial becomes the point; the caller swaps the buffers afterwards
  const int64_t P = f->P;
  double *gvec = f->redbuf + f->npk;
  f->r_fresh = true;      // f->r is the whitened residual AT p_trial: the trial evaluation left it there
  f->r_ptr = f->p_trial;
  int rc = eval_normal_dev(f, f->p_trial, false);
  if (rc) return rc;
  // (prior_deferred: g += Lambda (p - pbar), chi2 += ... inside the tail kernel -- one launch fewer)
  const bool wp = f->cfg.has_prior && f->adds_prior;
  HIPCHK(f, launch_lm_accept_tail(f->st, f->redbuf, P, f->opt.scaler, f->diag_dev, f->dscale, f->p_trial, f->yv + P, gvec,
                                  f->opt.xtol, f->opt.gtol, f->lmd, f->prior_deferred ? f->tvec : nullptr, f->prior_mean,
                                  f->nrm_in_tail ? f->nrm_part : nullptr, f->nrm_in_tail, (f->nrm_in_tail && wp) ? f->prior_prec : nullptr,
                                  f->cfg.prior_dense));
  return publish_record(f);
}

// run one half eagerly, or capture it (second time this parity sees it) and replay it
static int run_half(lsqamd_fit *f, int which, int (*enqueue)(lsqamd_fit *)) {
  static const bool env_off = [] { const char *e = getenv("LSQAMD_STEP_GRAPH"); return e && e[0] == '0'; }();
  static const int64_t maxp = [] { const char *e = getenv("LSQAMD_STEP_GRAPH_MAXP"); return e ? atoll(e) : (int64_t)1024; }();
  const bool eligible = !env_off && !f->step_graph_off && !f->timing && !f->comm && !f->reduce && f->P <= maxp;
  const int par = f->p_dev == f->p_buf0 ? 0 : 1;
  if (!eligible) return enqueue(f);
  hipGraphExec_t &exec = f->step_exec[par][which];
  if (!exec) {
    if (f->step_seen[par][which]++ == 0) return enqueue(f);      // warm-up: one-time attribute calls happen here
    const int64_t njev0 = f->njev;
    static const bool diag_capture = getenv("LSQAMD_FIT_DIAG") != nullptr;       // developer knob: how long do captures take?
    const auto tc0 = std::chrono::steady_clock::now();
    hipError_t e = hipStreamBeginCapture(f->st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      f->step_graph_off = true;
      return enqueue(f);
    }
    const int rc = enqueue(f);
    hipGraph_t gr = nullptr;
    e = hipStreamEndCapture(f->st, &gr);
    f->njev = njev0;                                             // counted when the graph runs, below
    if (rc || e != hipSuccess || !gr || hipGraphInstantiate(&exec, gr, nullptr, nullptr, 0) != hipSuccess) {
      if (gr) (void)hipGraphDestroy(gr);
      (void)hipGetLastError();
      exec = nullptr;
      f->step_graph_off = true;
      // enqueue failed AND the capture ended in error: the capture was invalidated (another thread's legacy-stream call, for
      // one) and took the captured launches down with it -- nothing ran; the half step is queued again, eagerly.  A failure
      // with a healthy capture is the enqueue's own
      if (rc && e == hipSuccess) return rc;
      capture_reset(f->st);      // (an invalidated capture leaves the stream unusable until it is reset: common.h)
      return enqueue(f);
    }
    (void)hipGraphDestroy(gr);
    if (diag_capture)
      fprintf(stderr, "lsqamd: captured + instantiated half-step graph [parity %d][%s] of handle %p in %.2f ms\n", par, which ? "accept" : "trial",
              (void *)f, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count());
  }
  HIPCHK(f, hipGraphLaunch(exec, f->st));
  f->graph_launches++;
  if (which == 1) note_accept_replayed(f);   // what enqueue_accept's host side does besides launching (eval.hip, next to eval_normal_dev)
  else f->r_fresh = false;
  return 0;
}

// The record of the half step just queued has arrived in pin_lm.  With the kernels mirroring it themselves (zero copy)
// the host POLLS the mirror's sequence number for a while before it falls back to a stream synchronisation: waking
// from the latter costs ~15 us of the ~27 us between two half steps of a small fit (LSQAMD_POLL=0: always synchronise).
static int wait_record(lsqamd_fit *f) {
  static const bool polling = [] { const char *e = getenv("LSQAMD_POLL"); return !(e && e[0] == '0'); }();
  f->lm_seq_expect += 1.0;
  if (!f->lm_zero_copy) {     // (the caller queued a copy of the record behind the kernels)
    HIPCHK(f, hipStreamSynchronize(f->st));
    return 0;
  }
  // The kernels' stores to the mirror arrive in no particular order (vecops.hip lm_publish): a snapshot counts only when its
  // sequence number is the awaited one AND its checksum fits.  Once one does, every word of this half step has landed and
  // nothing writes the mirror again before the host queues the next half step: the callers read pin_lm itself afterwards.
  volatile unsigned long long *h = reinterpret_cast<volatile unsigned long long *>(f->pin_lm);
  unsigned long long w[LMS_COUNT];
  auto arrived = [&]() {
    double seq;
    w[LMS_SEQ] = h[LMS_SEQ];
    std::memcpy(&seq, &w[LMS_SEQ], sizeof(double));
    if (!(seq >= f->lm_seq_expect)) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < LMS_COUNT; ++i) w[i] = h[i];
    std::memcpy(&seq, &w[LMS_SEQ], sizeof(double));
    if (seq >= f->lm_seq_expect && w[LMS_CHECK] == lm_record_checksum(w)) return true;
    g_handoff[0]++;
    return false;
  };
  auto audited = [&]() -> int {    // test knob: the record the host is about to act on vs the device's own, once the stream has drained
    if (!getenv("LSQAMD_VERIFY_HANDOFF")) return 0;
    unsigned long long dev[LMS_COUNT];
    HIPCHK(f, hipStreamSynchronize(f->st));
    HIPCHK(f, hipMemcpyAsync(dev, f->lmd, sizeof(dev), hipMemcpyDeviceToHost, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
    for (int i = 0; i < LMS_COUNT; ++i)
      if (dev[i] != w[i]) {
        fprintf(stderr, "lsqamd HANDOFF MISMATCH record word %d: host %016llx device %016llx\n", i, w[i], dev[i]);
        g_handoff[2]++;
      }
    return 0;
  };
  if (polling && poll(arrived, 3000)) return audited();
  HIPCHK(f, hipStreamSynchronize(f->st));
  if (arrived()) return audited();
  // the stream has drained and the mirror still does not verify: take the record from the device
  g_handoff[1]++;
  if (const int rc = fetch_record(f)) return rc;
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
}

// A trial with the step of the orthogonal factorisation (solver = qr, see iterate_device): the record goes back to mu0, nu0,
// delta0, then solve, trial point, residual and decision as in enqueue_trial.  No orthogonal factor either: rejected (mu grows)
static int qr_trial(lsqamd_fit *f, double mu0, long nu0, double delta0) {
  const int64_t P = f->P;
  double *rec = f->pin_lm;
  rec[LMS_MU] = mu0; rec[LMS_NU] = (double)nu0; rec[LMS_DELTA] = delta0;
  rec[LMS_ACCEPT] = 0.0; rec[LMS_SOLVED] = 0.0;
  HIPCHK(f, hipMemcpyAsync(f->lmd, rec, sizeof(double) * LMS_COUNT, hipMemcpyHostToDevice, f->st));
  int rc = solve_damped_qr(f, mu0);
  if (rc < 0 && rc != LSQAMD_ENOTPD && rc != LSQAMD_EUNSUPPORTED) return rc;
  if (rc != 0) {
    f->chol_fail++;
    rec[LMS_MU] = mu0 * (double)nu0; rec[LMS_NU] = 2.0 * (double)nu0;
    HIPCHK(f, hipMemcpyAsync(f->lmd, rec, sizeof(double) * LMS_COUNT, hipMemcpyHostToDevice, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
    return 0;
  }
  HIPCHK(f, launch_lm_trial(f->st, P, f->p_dev, f->yv + P, f->redbuf + f->npk, f->dscale, f->p_trial, f->lmd));
  if ((rc = eval_residual_launch(f, f->p_trial, true)) || (rc = publish_record(f)) || (rc = wait_record(f))) return rc;
  if (rec[LMS_SOLVED] != 0.0) f->qr_trials++;
  return 0;
}

int iterate_device(lsqamd_fit *f) {
  const int64_t P = f->P;
  double *gvec = f->redbuf + f->npk;
  int bad_steps = 0;
  while (true) {
    const double mu0 = f->mu, delta0 = f->delta;
    const long nu0 = f->nu;
    const double *st = f->pin_lm;
    static const bool qr_steps_off = [] { const char *e = getenv("LSQAMD_QR_STEPS"); return e && e[0] == '0'; }();   // developer knob
    const bool can_qr = f->opt.solver == LSQAMD_SOLVER_QR && f->qr_work && !f->comm && !f->reduce && !qr_steps_off;
    int rc = 0;
    bool need_qr = can_qr && f->qr_steps_on;
    if (!need_qr) {
      rc = run_half(f, 0, enqueue_trial);
      if (rc) return rc;
      rc = wait_record(f);
      if (rc) return rc;
      // solver = qr (the reference's default, src/lsqfit/_gsl.pyx:571,646-647): gsl factors [J ; sqrt(mu) D] itself, error
      // ~ cond eps; the damped normal equations have just gone through cond^2 ~ 1 / PIVMIN.  Once a trial's factor
      // retains less than 1e-8 of some column (or has no positive pivot at all), this fit's steps come from the
      // orthogonal factorisation (solve_damped_qr) -- the trial just taken included: the device's decision on it is
      // taken back (mu, nu, delta as before) and the trial is repeated with the accurate step
      if (can_qr && (st[LMS_SOLVED] == 0.0 || st[LMS_PIVMIN] < 1e-8)) {
        if (st[LMS_SOLVED] == 0.0) f->chol_fail++;
        f->qr_steps_on = true;
        need_qr = true;
      }
    }
    f->ntrial++;
    if (need_qr) {
      if ((rc = qr_trial(f, mu0, nu0, delta0))) return rc;
    } else if (st[LMS_SOLVED] == 0.0) {
      f->chol_fail++;
    }
    if (st[LMS_SOLVED] != 0.0) f->nfev++;   // (a residual evaluated at garbage is not a trial)
    f->mu = st[LMS_MU];
    f->nu = (long)st[LMS_NU];
    f->delta = st[LMS_DELTA];
    if (st[LMS_ACCEPT] != 0.0) {
      rc = run_half(f, 1, enqueue_accept);
      if (rc) return rc;
      std::swap(f->p_dev, f->p_trial);
      rc = wait_record(f);
      if (rc) return rc;
      f->chi2 = f->pin_lm[LMS_CHI2];
      f->conv_info_dev = (int32_t)f->pin_lm[LMS_INFO];
      if (!std::isfinite(f->chi2)) FAIL(f, LSQAMD_ENONFINITE, "chi2 is not finite at this point");
      return 0;
    }
    if (++bad_steps > 15) {
      // gsl_multifit_nlinear_driver tests convergence after an iteration that made no progress as
      // well, with the last (rejected) trial step as dx: at a minimum resolved to rounding that
      // step is below xtol and the fit ends on criterion 1
      HIPCHK(f, launch_lm_converge(f->st, P, f->p_dev, f->yv + P, gvec, f->opt.xtol, f->opt.gtol, f->lmd));
      if ((rc = publish_record(f))) return rc;
      rc = wait_record(f);
      if (rc) return rc;
      f->conv_info_dev = (int32_t)f->pin_lm[LMS_INFO];
      return LSQAMD_ENOPROG;
    }
  }
}

struct Proposal {   // trs->step + trs->preduction of one trial of the host-driven methods
  std::vector<double> dx, Adx;   // the step; scratch for A dx
  bool have_step = false;        // false: the damped matrix had no Cholesky factor -- the trial is rejected
  double pred_num = 0.0;         // predicted reduction * chi2
  double avratio = 0.0;          // lmaccel: |a| / |v|
  bool residual_done = false;    // plain lm: p_trial already holds x + dx and
  double chi2_t = 0.0;           //           chi2 there is this
};

// plain lm: everything up to the trial chi2 is queued without a host round trip -- solve, x_trial = x - v on the device,
// residual there; one synchronisation collects v, the factorisation status and chi2(x_trial).  -> the solve's status
static int lm_solve_and_try(lsqamd_fit *f, Proposal &s) {
  int rc = solve_damped_launch(f, f->mu, nullptr);
  if (rc) return rc;
  HIPCHK(f, launch_trial_point(f->st, f->P, f->p_dev, f->yv + f->P, f->p_trial));
  rc = eval_residual_dev(f, f->p_trial, &s.chi2_t);
  if (rc) return rc;
  rc = solve_damped_collect(f);
  if (rc == LSQAMD_ENOTPD) f->nfev--;  // that residual was evaluated at garbage: not a trial
  s.residual_done = rc == 0;
  return rc;
}

// geodesic acceleration (lm.c lm_step, fdfvv.c) on top of the velocity in s.dx, the factor of A + mu D^2 still in place:
// fvv by finite differences, h = 0.02; dx = v + a / 2, |a| / |v|, and lm_preduction on the corrected step
static int lmaccel_correct(lsqamd_fit *f, Proposal &s) {
  const int64_t P = f->P;
  const double h = 0.02;
  std::vector<double> vel(s.dx), xh(P), Gh(P), Av(P), rhs(P), acc(P);
  for (int64_t j = 0; j < P; ++j) xh[j] = f->hx[j] + h * vel[j];
  int rc = grad_like_at(f, xh.data(), Gh.data());
  if (rc || (rc = symv_host(f, vel.data(), Av.data()))) return rc;
  // J^T fvv = (2/h) ((G_h - g)/h - A v); the acceleration solves (A + mu D^2) a = -J^T fvv
  for (int64_t j = 0; j < P; ++j) rhs[j] = (2.0 / h) * ((Gh[j] - f->hg[j]) / h - Av[j]);
  rc = solve_with_factor(f, rhs.data(), acc.data());
  if (rc) return rc;
  double an = 0.0, vn = 0.0;
  for (int64_t j = 0; j < P; ++j) {
    const double a = -acc[j];
    an += a * a;
    vn += vel[j] * vel[j];
    s.dx[j] = vel[j] + 0.5 * a;
  }
  s.avratio = std::sqrt(an) / std::sqrt(vn);
  // lm_preduction on dx: |J dx|^2 + 2 mu |D dx|^2
  rc = symv_host(f, s.dx.data(), s.Adx.data());
  if (rc) return rc;
  const double dn = scaled_norm(f->hdiag, s.dx);
  s.pred_num = dot_h(s.dx, s.Adx) + 2.0 * f->mu * dn * dn;
  return 0;
}

// lm / lmaccel: the damped solve, dx = -v and its predicted reduction
static int propose_lm(lsqamd_fit *f, Proposal &s) {
  const int rc = f->opt.trs == LSQAMD_TRS_LM ? lm_solve_and_try(f, s) : solve_damped_dev(f, f->mu, f->hdiag.data());
  if (rc < 0 && rc != LSQAMD_ENOTPD) return rc;
  if (rc != 0) return 0;
  s.have_step = true;
  double vg = 0.0, dv2 = 0.0;
  for (int64_t j = 0; j < f->P; ++j) {
    s.dx[j] = -f->hv[j];
    vg += f->hv[j] * f->hg[j];
    const double t = f->hdiag[j] * f->hv[j];
    dv2 += t * t;
  }
  // |J v|^2 = v^T A v = v^T g - mu |D v|^2  since (A + mu D^2) v = g
  s.pred_num = vg + f->mu * dv2;
  return f->opt.trs == LSQAMD_TRS_LMACCEL ? lmaccel_correct(f, s) : 0;
}

// dogleg, ddogleg, subspace2D: the step for the current radius and quadratic_preduction, -(|J dx|^2 + 2 g.dx)
static int propose_legs(lsqamd_fit *f, Legs &L, Proposal &s) {
  int rc = legs_step(f, L, s.dx);
  if (rc || (rc = symv_host(f, s.dx.data(), s.Adx.data()))) return rc;
  s.have_step = true;
  s.pred_num = -(dot_h(s.dx, s.Adx) + 2.0 * dot_h(f->hg, s.dx));
  return 0;
}

// one trust_iterate: GSL_SUCCESS (0) or LSQAMD_ENOPROG; negative on backend failure
int iterate(lsqamd_fit *f) {
  if (f->dev_lm && f->opt.trs == LSQAMD_TRS_LM && f->linear.empty()) return iterate_device(f);
  if (f->mirrors_stale) {
    const int rcm = refresh_mirrors(f);
    if (rcm) return rcm;
  }
  f->dev_lm = false;
  if (!f->linear.empty()) return iterate_varpro(f);
  const int64_t P = f->P;
  const int trs = f->opt.trs;
  const bool lm_family = trs == LSQAMD_TRS_LM || trs == LSQAMD_TRS_LMACCEL;
  int bad_steps = 0;
  std::vector<double> xt(P);
  Proposal s;
  s.dx.resize(P); s.Adx.resize(P);
  Legs L;
  if (!lm_family) {
    const int rc = legs_preloop(f, L);
    if (rc) return rc;
  }
  while (true) {
    s.have_step = s.residual_done = false;
    s.pred_num = s.avratio = s.chi2_t = 0.0;
    int rc = lm_family ? propose_lm(f, s) : propose_legs(f, L, s);
    if (rc) return rc;
    double rho = -1.0;
    if (s.have_step) {
      for (int64_t j = 0; j < P; ++j) {
        f->hdx[j] = s.dx[j];
        xt[j] = f->hx[j] + s.dx[j];
      }
      if (!s.residual_done && (rc = trial_residual(f, xt.data(), &s.chi2_t))) return rc;
      rho = gain_ratio(f->chi2, s.chi2_t, s.pred_num);
    }
    if (rho > 0.75) f->delta *= f->opt.factor_up;
    else if (rho < 0.25) f->delta /= f->opt.factor_down;
    // trust_eval_step: with geodesic acceleration the step must also satisfy |a|/|v| <= avmax
    if (rho > 0.0 && !(trs == LSQAMD_TRS_LMACCEL && s.avratio > f->opt.avmax)) {
      if ((rc = accept_trial(f, xt, true))) return rc;
      nielsen_accept(f, rho);
      return 0;
    }
    nielsen_reject(f);
    if (++bad_steps > 15) return LSQAMD_ENOPROG;
  }
}

int convergence_test(lsqamd_fit *f) {
  if (f->dev_lm) return f->conv_info_dev;
  const int64_t P = f->P;
  const double xtol = f->opt.xtol, gtol = f->opt.gtol;
  bool ok = true;
  for (int64_t j = 0; j < P; ++j)
    if (!(std::fabs(f->hdx[j]) < xtol * xtol + xtol * std::fabs(f->hx[j]))) { ok = false; break; }
  if (ok) return 1;
  double gnorm = 0.0;
  for (int64_t j = 0; j < P; ++j) {
    const double t = std::fabs(std::fmax(f->hx[j], 1.0) * f->hg[j]);
    if (t > gnorm) gnorm = t;
  }
  if (gnorm <= gtol * std::fmax(0.5 * f->chi2, 1.0)) return 2;
  return 0;
}

// nonlinear_fit's linear= (lsqamd_set_linear): variable projection (iterate_varpro) starts from the projected point --
// A_aa da = -g_a with the others frozen, one more evaluation
static int varpro_start(lsqamd_fit *f) {
  const int64_t P = f->P;
  std::vector<double> frozen(P);
  for (int64_t j = 0; j < P; ++j) frozen[j] = f->linear[j] ? 0.0 : 1.0;
  int rc = solve_damped_dev(f, 0.0, nullptr, frozen.data());
  if (rc == LSQAMD_ENOTPD) FAIL(f, LSQAMD_ENOTPD, "linear parameters: their block of J^T J is not positive definite");
  if (rc) return rc;
  for (int64_t j = 0; j < P; ++j)
    if (f->linear[j]) f->hx[j] -= f->hv[j];
  if ((rc = upload_point(f, f->p_dev, f->hx.data())) || (rc = eval_normal_dev(f, f->p_dev))) return rc;
  f->nfev++;
  return 0;
}

// plain lm on the device: the record its decisions start from (once per fit), from the handle's chi2, mu, nu, delta
static int start_device_record(lsqamd_fit *f) {
  for (int i = 0; i < LMS_COUNT; ++i) f->pin_lm[i] = 0.0;
  f->pin_lm[LMS_CHI2] = f->chi2; f->pin_lm[LMS_MU] = f->mu; f->pin_lm[LMS_NU] = (double)f->nu;
  f->pin_lm[LMS_DELTA] = f->delta;
  // the kernels that finish a half step mirror the record into this pinned block themselves (LSQAMD_ZERO_COPY=0: a copy per read)
  const char *zc = getenv("LSQAMD_ZERO_COPY");      // (read per call: a tested mode)
  const bool off = zc && zc[0] == '0';
  void *dp = nullptr;
  f->lm_zero_copy = !off && hipHostGetDevicePointer(&dp, f->pin_lm, 0) == hipSuccess && dp != nullptr;
  if (!f->lm_zero_copy) (void)hipGetLastError();
  long long bits = f->lm_zero_copy ? (long long)(intptr_t)dp : 0;
  std::memcpy(&f->pin_lm[LMS_HOSTPTR], &bits, sizeof(double));
  f->lm_seq_expect = 0.0;
  HIPCHK(f, hipMemcpyAsync(f->lmd, f->pin_lm, sizeof(double) * LMS_COUNT, hipMemcpyHostToDevice, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
}

int do_init(lsqamd_fit *f, const double *p0) {
  int rc = ready(f);
  if (rc) return rc;
  const int64_t P = f->P;
  if (!f->linear.empty() && f->opt.trs != LSQAMD_TRS_LM)
    FAIL(f, LSQAMD_EINVAL, "linear parameters (lsqamd_set_linear) need the plain lm method");
  f->hx.assign(p0, p0 + P);
  f->hg.assign(P, 0.0);
  f->hdiag.assign(P, 1.0);
  f->hdx.assign(P, 0.0);
  f->hv.assign(P, 0.0);
  f->hcoln.assign(P, 0.0);
  f->nit = f->nfev = f->njev = f->ntrial = f->chol_fail = f->qr_trials = 0;
  f->qr_steps_on = false;
  f->logdet = NAN;
  HIPCHK(f, hipMemcpyAsync(f->p_dev, p0, sizeof(double) * P, hipMemcpyHostToDevice, f->st));
  rc = eval_normal_dev(f, f->p_dev);
  if (rc) return rc;
  f->nfev++;
  if (!f->linear.empty() && (rc = varpro_start(f))) return rc;
  scale_init(f);
  double mx = 0.0;   // over the damped parameters (all of them unless lsqamd_set_linear was used)
  for (int64_t j = 0; j < P; ++j)
    if (f->linear.empty() || !f->linear[j]) mx = std::fmax(mx, f->hcoln[j] / f->hdiag[j]);
  f->mu = 1e-3 * mx * mx;
  f->nu = 2;
  double dxn = 0.0;
  for (int64_t j = 0; j < P; ++j) dxn += f->hdiag[j] * f->hx[j] * f->hdiag[j] * f->hx[j];
  f->delta = 0.3 * std::fmax(1.0, std::sqrt(dxn));
  f->mirrors_stale = false;
  f->conv_info_dev = 0;
  f->dev_lm = f->opt.trs == LSQAMD_TRS_LM && f->linear.empty() && getenv("LSQAMD_HOST_LM") == nullptr;
  if (f->dev_lm && (rc = start_device_record(f))) return rc;
  f->initialised = true;
  return 0;
}

// One pass of gsl_multifit_nlinear_driver's loop: trust_iterate, nit, the convergence test -> 0 with *info the criterion
// met (0: none).  An iteration without progress is tested like any other unless stall_ends: then LSQAMD_ENOPROG, *info too
int driver_iteration(lsqamd_fit *f, int *info, bool stall_ends) {
  const int rc = iterate(f);
  if (rc < 0) return rc;
  f->nit++;
  if (rc == LSQAMD_ENOPROG && stall_ends) {
    *info = LSQAMD_ENOPROG;
    return LSQAMD_ENOPROG;
  }
  *info = convergence_test(f);
  return 0;
}

// gsl_multifit_nlinear_init + _driver (src/lsqfit/_gsl.pyx:676-677) from p0.  *info as driver_iteration leaves it (0 without
// an iteration); *status 0: converged, or maxit < 1; LSQAMD_EMAXITER: out of iterations, or the first one made no progress
int run_gsl_driver(lsqamd_fit *f, const double *p0, int *status, int *info) {
  int rc = do_init(f, p0);
  if (rc) return rc;
  const int maxit = f->opt.maxit;
  *status = 0;
  if (maxit <= 0) return 0;
  int iter = 0;
  do {
    rc = driver_iteration(f, info, iter == 0);
    if (rc < 0) return rc;
    if (rc == LSQAMD_ENOPROG) {
      *status = LSQAMD_EMAXITER;
      return 0;
    }
    ++iter;
    *status = *info ? 0 : -2;
  } while (*status == -2 && iter < maxit);
  if (iter >= maxit && *status != 0) *status = LSQAMD_EMAXITER;
  return 0;
}

void fill_summary(lsqamd_fit *f, lsqamd_summary *s, int status, int info) {
  if (!s) return;
  std::memset(s, 0, sizeof(*s));
  s->status = status;
  s->info = info;
  if (info >= 0 && info <= 3) s->stopping_criterion = info;
  else if (info == 30) s->stopping_criterion = 1;
  else if (info == 31) s->stopping_criterion = 2;
  else if (info == 29) s->stopping_criterion = 3;
  else if (info == 27) s->stopping_criterion = 4;
  else if (info >= LSQAMD_INFO_TRF && info <= LSQAMD_INFO_TRF + 4) {
    static const int map[5] = {0, 2, 3, 1, 1};   // _scipy.py:176-181
    s->stopping_criterion = map[info - LSQAMD_INFO_TRF];
  } else s->stopping_criterion = 0;
  s->nit = f->nit; s->nfev = f->nfev; s->njev = f->njev; s->ntrial = f->ntrial;
  s->chol_fail = f->chol_fail;
  s->qr_trials = f->qr_trials;
  s->chi2 = f->chi2;
  s->mu = f->mu;
  s->logdet_jtj = f->logdet;
}

// A whole small fit in ONE launch (jit.hip lsqamd_jit_lm): a compiled formula with at most a dozen parameters, uncorrelated rows,
// a few thousand of them at most, plain lm on one rank -- the fits of examples/nist.py and tests/test_lsqfit.py, where the
// half dozen launches and two host round trips of an iteration of iterate_device cost more than its arithmetic.  One workgroup
// runs gsl_multifit_nlinear_init + _driver (src/lsqfit/_gsl.pyx:676-677) from p0 to the stopping criterion -- and, for the
// normal-equation route, gsl_multifit_nlinear_covar (:706) -- and hands back the state where do_init / iterate_device
// would have left it (device buffers and host mirrors).  Here in stages: who takes the route, the kernel's arguments, the wait
// for its record block, the block's audit, its adoption into the handle; run_one_launch at the end.
using namespace lsqamd_jit;   // (the record block's layout: FIT_REC_*, fit_host_diag, fit_host_cov)

struct FitLaunch {   // one launch of the fit kernel
  void *dfit = nullptr, *dx = nullptr, *dlm = nullptr;   // the device's addresses of pin_fit, pin_x, pin_lm
  bool zero_copy = true;                                 // the kernel publishes its record block to pin_fit
  unsigned long long seq = 0;                            // how the host tells this launch's block from an earlier one's
  int nw = 0;                                            // words of the record block of a P-parameter fit
};

static bool one_launch_eligible(const lsqamd_fit *f) {
  const char *e = getenv("LSQAMD_ONE_LAUNCH_FIT");
  if (e && e[0] == '0') return false;
  const Kernel *k = static_cast<const Kernel *>(f->jit);
  if (!has_fit_kernel(k) || f->P > FIT_MAX_P || f->N < 1 || f->N > fit_row_limit(k, f->cfg.n_blocks != 0)) return false;
  if (f->opt.trs != LSQAMD_TRS_LM || !f->linear.empty() || getenv("LSQAMD_HOST_LM") || f->opt.maxit < 1) return false;
  if (f->opt.maxit > 20000) return false;  // (a kernel cannot be interrupted: runs of that length stay on the host-driven path)
  if (f->comm || f->reduce || f->timing || !small_fuse(f) || !f->progs.empty() || f->have_param_rows) return false;
  // correlated rows: the workgroup whitens them itself (one row per thread, the raw rows in LDS) -- up to 256 rows in all
  if (f->cfg.n_blocks > 64) return false;
  return !(f->cfg.has_prior && !f->adds_prior);
}

static FitArgs fit_args(const lsqamd_fit *f, const FitLaunch &L) {
  const int64_t P = f->P;
  FitArgs a;
  a.x = f->x; a.ymean = f->ymean; a.wdiag = f->wdiag; a.n_data = f->N;
  a.in_block = f->in_block; a.wt = f->wt;
  a.blk_row0 = reinterpret_cast<const long long *>(f->blk_row0); a.blk_size = reinterpret_cast<const long long *>(f->blk_size);
  a.blk_woff = reinterpret_cast<const long long *>(f->blk_woff); a.n_blocks = f->cfg.n_blocks;
  a.p0 = static_cast<const double *>(L.dx);
  a.p = f->p_dev; a.p_trial = f->p_trial; a.dscale = f->dscale; a.apk = f->redbuf; a.gvec = f->redbuf + f->npk;
  a.v_out = f->yv + P; a.coln2 = f->diag_dev; a.st = f->lmd;
  a.prior_prec = f->cfg.has_prior ? f->prior_prec : nullptr;
  a.prior_mean = f->cfg.has_prior ? f->prior_mean : nullptr;
  a.prior_dense = f->cfg.prior_dense; a.scaler = f->opt.scaler; a.maxit = f->opt.maxit;
  a.watch = f->opt.solver == LSQAMD_SOLVER_QR ? 1 : 0;
  a.xtol = f->opt.xtol; a.gtol = f->opt.gtol; a.factor_up = f->opt.factor_up; a.factor_down = f->opt.factor_down;
  // LSQAMD_ZERO_COPY=0: nothing is published to host memory; the host waits for the stream and copies the kernel's device
  // block -- also what happens when a published block does not verify in time
  const long long bits = L.zero_copy ? (long long)(intptr_t)L.dlm : 0;
  std::memcpy(&a.hostptr_bits, &bits, sizeof(double));
  a.host = f->fit_block;
  a.pub = L.zero_copy ? static_cast<unsigned long long *>(L.dfit) : nullptr;
  a.seq = L.seq;
  // the covariance of the normal-equation route rides along (solver = qr factors the Jacobian itself: do_covariance_qr)
  a.cov = f->cov; a.ldc = f->ldm; a.want_cov = f->opt.solver == LSQAMD_SOLVER_QR ? 0 : 1; a.pad_ = 0;
  return a;
}

// The launch's record block -> f->fit_rec.  A published block (zero copy) is polled for: the flag word is this launch's only when
// it carries this launch's sequence number; the block behind it counts only when its checksum (seeded with the same number)
// fits the snapshot taken -- the kernel's stores arrive in no particular order (jit.hip, end of lm_fit).  A short spin (most
// small fits end within 100 us), then yielding the core, then the stream; a block that still does not verify once the
// stream has drained, like one that was never published, is the device's copy.
static int await_fit_record(lsqamd_fit *f, const FitLaunch &L) {
  const int nw = L.nw;
  const unsigned long long seq = L.seq;
  f->fit_rec.resize((size_t)nw);
  volatile unsigned long long *hw = reinterpret_cast<volatile unsigned long long *>(f->pin_fit);
  unsigned long long *rec = reinterpret_cast<unsigned long long *>(f->fit_rec.data());
  auto arrived = [&]() {
    const unsigned long long flag = hw[FIT_REC_REASON];
    if ((flag >> 40) != seq) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < nw; ++i) rec[i] = hw[i];
    if (rec[FIT_REC_REASON] != flag || rec[FIT_REC_CHECK] != fit_checksum(rec, nw, seq)) { g_handoff[0]++; return false; }
    // the flag IS the decision: reason | info | nit; the record behind it must say the same
    const int reason = (int)(flag & 0xff), info = (int)(int8_t)((flag >> 8) & 0xff), nit = (int)((flag >> 16) & 0xffffff);
    if ((int)f->fit_rec[LMS_INFO] != info || (int)f->fit_rec[FIT_REC_NIT] != nit) { g_handoff[0]++; return false; }
    f->fit_rec[FIT_REC_REASON] = (double)reason;
    f->fit_rec[FIT_REC_CHECK] = 0.0;
    return true;
  };
  bool have = false;
  if (L.zero_copy) {
    have = poll(arrived, 5000);
    if (!have) {
      HIPCHK(f, hipStreamSynchronize(f->st));
      have = arrived();
      if (!have) g_handoff[1]++;
    }
  }
  if (!have) {
    HIPCHK(f, hipStreamSynchronize(f->st));
    HIPCHK(f, hipMemcpyAsync(f->fit_rec.data(), f->fit_block, sizeof(double) * (size_t)nw, hipMemcpyDeviceToHost, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
  }
  return 0;
}

// LSQAMD_VERIFY_HANDOFF (test knob): the block the host acted on vs the device's own copy once the stream has drained
static int audit_fit_record(lsqamd_fit *f, int nw) {
  std::vector<double> dev((size_t)nw);
  HIPCHK(f, hipStreamSynchronize(f->st));
  HIPCHK(f, hipMemcpyAsync(dev.data(), f->fit_block, sizeof(double) * (size_t)nw, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  int bad = 0;
  for (int i = 0; i < nw; ++i)
    if (i != FIT_REC_CHECK && std::memcmp(&dev[(size_t)i], &f->fit_rec[(size_t)i], sizeof(double)) != 0) {
      fprintf(stderr, "lsqamd HANDOFF MISMATCH word %d: host %a device %a\n", i, f->fit_rec[(size_t)i], dev[(size_t)i]);
      ++bad;
    }
  if (bad) {
    g_handoff[2] += bad;
    fprintf(stderr, "lsqamd HANDOFF: %d mismatches (P %lld N %lld)\n", bad, (long long)f->P, (long long)f->N);
  }
  return 0;
}

// A finished fit's record block (f->fit_rec) into the handle: the host mirrors, the LM record, the counters, the flags as
// do_init / iterate_device would have left them, the covariance's state
static void adopt_fit_record(lsqamd_fit *f, bool zero_copy, bool want_cov) {
  const int64_t P = f->P;
  const double *R = f->fit_rec.data();
  const double *m = R + FIT_REC_MIRRORS;
  f->hx.assign(m, m + P);
  f->hg.assign(m + (P + 1), m + (P + 1) + P);
  f->hdiag.assign(m + 2 * (P + 1), m + 2 * (P + 1) + P);
  f->hcoln.resize(P); f->hv.resize(P); f->hdx.resize(P);
  for (int64_t j = 0; j < P; ++j) {
    const double c2 = m[3 * (P + 1) + j], v = m[4 * (P + 1) + j];
    f->hcoln[j] = std::sqrt(c2 > 0.0 ? c2 : 0.0);
    f->hv[j] = v;
    f->hdx[j] = -v;
  }
  for (int i = 0; i < LMS_COUNT; ++i) f->pin_lm[i] = R[i];
  f->nit = (int)R[FIT_REC_NIT]; f->nfev = (int)R[FIT_REC_NFEV]; f->njev = (int)R[FIT_REC_NJEV]; f->ntrial = (int)R[FIT_REC_NTRIAL];
  f->chol_fail = f->qr_trials = 0;
  f->qr_steps_on = false;
  f->logdet = NAN;
  f->chi2 = R[LMS_CHI2]; f->mu = R[LMS_MU]; f->nu = (long)R[LMS_NU]; f->delta = R[LMS_DELTA];
  f->conv_info_dev = (int32_t)R[LMS_INFO];
  f->dev_lm = true;
  f->lm_zero_copy = zero_copy;
  f->lm_seq_expect = 0.0;
  f->mirrors_stale = false;
  f->J_stale = true;               // (no Jacobian was written: ensure_J() for whoever reads it)
  f->used_nrm = true;
  f->used_one_launch = true;
  if (getenv("LSQAMD_FIT_DIAG")) {   // developer knob: where the kernel's cycles went
    const double *c = R + fit_host_diag((int)P);
    fprintf(stderr, "lsqamd_jit_lm: %.0f shader cycles (normal equations %.0f, solves %.0f, trial residuals %.0f), %.1f us; nit %d trials %d\n",
            c[0], c[1], c[2], c[3], c[4] / 100.0, (int)f->nit, (int)f->ntrial);
  }
  f->nrm_in_tail = 0;
  f->prior_deferred = false;
  f->r_fresh = false;
  f->have_cov = false;
  f->cov_host_valid = false;
  if (want_cov && R[FIT_REC_HAVE_COV] == 1.0) {     // (else: do_covariance, the caller's next step)
    f->have_cov = true;
    f->cov_host_valid = true;
    f->cov_inaccurate = false;
    f->cov_dropped = 0;
    f->logdet = R[FIT_REC_LOGDET];
  }
  f->have_dense_A = false;
  f->initialised = true;
}

// -> 1: done (*info: the criterion met, 0 none; *status: 0, -2 or LSQAMD_EMAXITER as the driver loop would have left it); 0: not
// this fit's route, or the kernel met something irregular and the general path runs the fit from the start; < 0: error.
// LSQAMD_ONE_LAUNCH_FIT=0 disables, LSQAMD_ZERO_COPY=0 keeps the record block off host memory (both read per call: tested modes)
int run_one_launch(lsqamd_fit *f, const double *p0, int *status, int *info) {
  if (!one_launch_eligible(f)) return 0;
  int rc = ready(f);
  if (rc) return rc;
  FitLaunch L;
  if (!f->fit_block || hipHostGetDevicePointer(&L.dfit, f->pin_fit, 0) != hipSuccess || hipHostGetDevicePointer(&L.dx, f->pin_x, 0) != hipSuccess ||
      hipHostGetDevicePointer(&L.dlm, f->pin_lm, 0) != hipSuccess || !L.dfit || !L.dx || !L.dlm) {
    (void)hipGetLastError();
    return 0;
  }
  const char *z = getenv("LSQAMD_ZERO_COPY");
  L.zero_copy = !(z && z[0] == '0');
  L.nw = fit_host_cov((int)f->P) + (int)(f->P * f->P);
  static std::atomic<unsigned> g_seq{0};
  while (L.seq == 0) L.seq = (g_seq.fetch_add(1, std::memory_order_relaxed) + 1u) & 0xffffffu;   // 24 bits, never 0
  std::memcpy(f->pin_x, p0, sizeof(double) * f->P);
  if (poison_pinned()) poison_fill(f->pin_fit, sizeof(double) * FIT_HOST_DOUBLES);
  reinterpret_cast<volatile unsigned long long *>(f->pin_fit)[FIT_REC_REASON] = 0;   // no flag yet
  std::atomic_thread_fence(std::memory_order_release);
  const Kernel *k = static_cast<const Kernel *>(f->jit);
  const FitArgs a = fit_args(f, L);
  HIPCHK(f, lsqamd_jit::launch_fit(k, f->st, a));
  if ((rc = await_fit_record(f, L))) return rc;
  if (getenv("LSQAMD_VERIFY_HANDOFF") && (rc = audit_fit_record(f, L.nw))) return rc;
  if (f->fit_rec[FIT_REC_REASON] != 1.0) {                 // irregular: the general path from the start
    HIPCHK(f, hipStreamSynchronize(f->st));
    return 0;
  }
  adopt_fit_record(f, L.zero_copy, a.want_cov != 0);
  *info = f->conv_info_dev;
  *status = *info ? 0 : ((int)f->nit >= f->opt.maxit ? LSQAMD_EMAXITER : -2);
  return 1;
}

}  // namespace lsqamd_host
