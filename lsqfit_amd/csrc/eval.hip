// The device evaluation blocks of a fit as launch sequences (gfx950 build, host code only; the kernels are in model.hip,
// whiten.hip, gemm_tn_f64.hip, vecops.hip, chol.hip, robust.hip, jit.hip): the whitened residual and chi2
// (eval_residual_*), the whitening of the Jacobian's block rows (whiten_jacobian), the normal equations J^T J, J^T f, chi2
// with their sum over the ranks (eval_normal_dev, a driver over named stages), the damped solve (solve_damped_*), the
// scaling matrix, the pieces the trust-region sub-problem solvers share (symv_host, solve_with_factor, grad_like_at),
// the host mirrors, log det and the covariance.  The drivers that queue them are lm_driver.hip and scipy_methods.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host.h"

using namespace lsqamd;

namespace lsqamd_host {

int do_reduce(lsqamd_fit *f, double *buf, int64_t count) {
  if (f->comm) {   // RCCL on the handle's stream: nothing to wait for on the host
    Scope sc(f, LSQAMD_T_REDUCE);
    Scope sc2(f, LSQAMD_T_EXCH_COLL, nullptr, LSQAMD_T_EXCH_WAIT);   // on the step's own stream: ONE interval, all of it waited for
    return comm_all_reduce(f, buf, count);
  }
  if (!f->reduce) return 0;
  Scope sc(f, LSQAMD_T_REDUCE);
  HIPCHK(f, hipStreamSynchronize(f->st));
  const int rc = f->reduce(f->reduce_user, buf, count);
  if (rc != 0) FAIL(f, LSQAMD_EREDUCE, "all-reduce hook returned %d", rc);
  return 0;
}

// whitened residual VECTOR at device parameters p -> f->r (model kernel + block whitening); launches only
static int residual_vector_launch(lsqamd_fit *f, const double *p) {
  ModelArgs m = model_args(f, p);
  if (f->cfg.model == LSQAMD_MODEL_COSMIX && f->have_x && trig_split_pays(f)) {
    // cosine model: the range flag of THIS point (the frequencies are parameters P/2 .. P - 1); the fused
    // whitening kernel, which only ever runs at the point whose residual is current, reads the same flag
    HIPCHK(f, launch_trig_range(f->st, p + f->P / 2, f->P / 2, f->xmax, f->trig_far));
    m.trig_far = f->trig_far;
  }
  HIPCHK(f, launch_residual_ex(f->st, m, f->r, f->r_raw));
  if (f->have_param_rows)
    HIPCHK(f, launch_param_rows(f->st, f->row_param, f->N, f->P, 1, p, f->ymean, f->wdiag,
                                f->cfg.n_blocks > 0 ? f->in_block : nullptr, f->r, f->r_raw, 0));
  if (f->cfg.n_blocks > 0) {
    // small blocks: one thread per output row; large ones (a single 8192-row block would keep
    // 32 workgroups busy for milliseconds): r_b = Wt_b^T delta_b as a two-stage column sum at
    // HBM speed, staged through the raw-Jacobian buffer (idle during a residual evaluation)
    constexpr int64_t BIG = 1024;
    HIPCHK(f, launch_block_whiten_vec(f->st, f->wt, f->blk_row0, f->blk_size, f->blk_woff,
                                      f->cfg.n_blocks, f->cfg.max_block, f->r_raw, f->r, 1, 0, nullptr, BIG));
    for (size_t b = 0; b < f->h_size.size(); ++b) {
      const int64_t B = f->h_size[b];
      if (B < BIG) continue;
      int64_t nch = (f->N * f->ld) / B;
      if (nch > 256) nch = 256;
      HIPCHK(f, launch_colsum_dot(f->st, f->wt + f->h_woff[b], B, B, B, 0, f->Jraw, nch,
                                  f->r + f->h_row0[b], f->r_raw + f->h_row0[b], 1, f->h_tri[b] ? 1 : 0));
    }
  }
  return 0;
}

// whitened residual at device parameters p -> f->r; chi2 (summed over ranks) -> f->red_scalar[0].
// Launches only: nothing is waited for.
// decide: a single rank's trial -- the sum of squares' second stage, the prior's share and the LM decision in
// one launch (lm_trial_tail_kernel); with ranks to sum over the scalar is exchanged first and the caller decides
int eval_residual_launch(lsqamd_fit *f, const double *p, bool decide) {
  f->r_fresh = false;
  if (decide) {
    Scope sc(f, LSQAMD_T_RESIDUAL);
    const int rc = residual_vector_launch(f, p);
    if (rc) return rc;
    const bool wp = f->cfg.has_prior && f->adds_prior;
    if (small_fuse(f) && f->N <= 65536 && !(wp && f->cfg.prior_dense)) {
      HIPCHK(f, launch_lm_trial_tail_small(f->st, f->r, f->N, f->P, wp ? f->prior_prec : nullptr, f->prior_mean, p, f->tvec,
                                           f->red_scalar, f->info_dev, f->opt.factor_up, f->opt.factor_down, f->lmd));
      return 0;
    }
    HIPCHK(f, launch_lm_trial_tail(f->st, f->r, f->N, f->partial, f->P, f->prior_prec, f->cfg.prior_dense,
                                   f->prior_mean, p, f->tvec, f->cfg.has_prior && f->adds_prior, f->red_scalar,
                                   f->info_dev, f->opt.factor_up, f->opt.factor_down, f->lmd));
    return 0;
  }
  {
    Scope sc(f, LSQAMD_T_RESIDUAL);
    const int rc = residual_vector_launch(f, p);
    if (rc) return rc;
    if (f->robust())    // scipy's loss_function(f, cost_only=True), as 2 x cost
      HIPCHK(f, launch_robust_cost(f->st, f->r, f->N, 1, f->loss, f->f_scale, f->partial, f->red_scalar));
    else
      HIPCHK(f, launch_sumsq(f->st, f->r, f->N, f->partial, f->red_scalar));
    if (f->cfg.has_prior && f->adds_prior)
      HIPCHK(f, launch_prior_chi2(f->st, f->P, f->prior_prec, f->cfg.prior_dense, f->prior_mean, p,
                                  f->tvec, f->red_scalar));
  }
  return do_reduce(f, f->red_scalar, 1);
}

// whitened residual at device parameters p -> f->r ; chi2 (all ranks) on return
int eval_residual_dev(lsqamd_fit *f, const double *p, double *chi2_out) {
  int rc = eval_residual_launch(f, p);
  if (rc) return rc;
  HIPCHK(f, hipMemcpyAsync(f->pin_s, f->red_scalar, sizeof(double), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  *chi2_out = f->pin_s[0];
  f->nfev++;
  return 0;
}

// ---- whitening of the block rows of the Jacobian (and of its residual column) ------------------------------------------
// uniform blocks: J_b = Wt_b^T Jraw_b over the columns [J | f] as ONE batched product
static GemmTN uniform_whitening_product(const lsqamd_fit *f) {
  const int64_t B = f->h_size[0];
  GemmTN g;
  g.X = f->wt; g.ldx = B; g.sx = B * B;
  g.Y = f->Jraw + f->h_row0[0] * f->ld; g.ldy = f->ld; g.sy = B * f->ld;
  g.C = f->J + f->h_row0[0] * f->ld; g.ldc = f->ld; g.sc = B * f->ld;
  g.M = B; g.N = f->P + 1; g.K = B;
  g.batch = f->cfg.n_blocks;
  g.x_upper_tri = f->uniform_tri;
  return g;
}

// full-tile uniform blocks: the residual column on its own, BEFORE the bulk (whose epilogue can then form its share of
// J^T f from the tile it still holds)
static int whiten_residual_column(lsqamd_fit *f, const GemmTN &g, bool r_here) {
  const int64_t B = f->h_size[0];
  // the residual column of a large block is a GEMV: two-stage column sum at HBM speed
  // (as a one-column GEMM it would keep B/128 workgroups busy for over a millisecond)
  int64_t nch = B >= 1024 ? (int64_t)f->splits * f->P * f->ldm / B : 0;
  if (nch > 256) nch = 256;
  if (nch >= 1) {
    for (int b = 0; b < f->cfg.n_blocks; ++b) {
      const int64_t r0 = f->h_row0[b];
      if (!r_here)   // (else f->r already holds the whitened residual of this point: the trial evaluation left it)
        HIPCHK(f, launch_colsum_dot(f->st, f->wt + f->h_woff[b], B, B, B, 0, f->slabs, nch, f->r + r0,
                                    f->Jraw + r0 * f->ld + f->P, f->ld, f->uniform_tri ? 1 : 0));
      HIPCHK(f, launch_copy_strided(f->st, f->r + r0, 1, f->J + r0 * f->ld + f->P, f->ld, B, 1));
    }
    return 0;
  }
  GemmTN c = g;
  c.Y += f->P; c.C += f->P; c.N = 1;
  HIPCHK(f, launch_gemm_tn(f->st, c));
  return 0;
}

// full-tile uniform blocks: what the bulk product (g, columns 0 .. P - 1) does besides whitening.  Either its epilogue leaves
// per-tile-row pieces of J^T f in the slabs (*fused_chunks of them), or -> true -- one (or a few) large blocks, too few
// workgroups for the chip -- it runs both halves of every tile row's K-range at once, the upper halves into the slabs (free
// until the J^T J launch) for the caller to add; J^T f then comes from that launch's diagonal tiles.  Or neither.
static bool choose_bulk_epilogue(const lsqamd_fit *f, GemmTN &g, bool plain, int64_t *fused_chunks) {
  const int64_t B = f->h_size[0], nb = f->cfg.n_blocks;
  const int64_t slab_doubles = (int64_t)f->splits * f->P * f->ldm;
  const bool all_rows = f->h_row0[0] == 0 && nb * B == f->N;
  const int64_t chunks = nb * (B / 128);
  if (!plain && all_rows && chunks * f->P <= slab_doubles) {
    g.colsum_out = f->slabs;
    g.colsum_ld = f->P;
    g.colsum_rcol = f->P;
    if (gemm_tn_fuses_colsum(g)) *fused_chunks = chunks;
    else g.colsum_out = nullptr;
  }
  if (nb * B * f->ld <= slab_doubles && all_rows) {
    GemmTN h = g;
    h.colsum_out = nullptr;
    h.tri_halves = 1;
    h.split_stride = f->slabs - g.C;
    if (gemm_tn_wants_tri_halves(h)) {
      g = h;
      *fused_chunks = 0;
      return true;
    }
  }
  return false;
}

// blocks of any sizes: one product per block, the residual column included
static int whiten_per_block(lsqamd_fit *f) {
  for (int b = 0; b < f->cfg.n_blocks; ++b) {
    const int64_t B = f->h_size[b];
    GemmTN g;
    g.X = f->wt + f->h_woff[b]; g.ldx = B;
    g.Y = f->Jraw + f->h_row0[b] * f->ld; g.ldy = f->ld;
    g.C = f->J + f->h_row0[b] * f->ld; g.ldc = f->ld;
    g.M = B; g.N = f->P + 1; g.K = B;
    g.x_upper_tri = f->h_tri[b];
    HIPCHK(f, launch_gemm_tn(f->st, g));
  }
  return 0;
}

// Whitening of the block rows of the Jacobian (and of its residual column).  *fused_chunks > 0 on
// return: the bulk GEMM also left per-tile-row partial sums of J^T f in f->slabs, reduced here into
// [J^T f | |f|^2] before the SYRK reuses the slabs.
// plain: no J^T f out of the product's epilogue (the rows are rescaled afterwards)
static int whiten_jacobian(lsqamd_fit *f, int64_t *fused_chunks, bool r_here, bool plain = false) {
  *fused_chunks = 0;
  if (f->cfg.n_blocks <= 0) return 0;
  Scope sc(f, LSQAMD_T_WHITEN);
  if (!f->uniform_blocks) return whiten_per_block(f);
  GemmTN g = uniform_whitening_product(f);
  if (!(f->P % 128 == 0 && f->h_size[0] % 128 == 0)) {   // ragged tiles: the general kernel, all P + 1 columns at once
    HIPCHK(f, launch_gemm_tn(f->st, g));
    return 0;
  }
  const int rc = whiten_residual_column(f, g, r_here);
  if (rc) return rc;
  g.N = f->P;   // full-tile bulk (interior kernel)
  const bool halves = choose_bulk_epilogue(f, g, plain, fused_chunks);
  HIPCHK(f, launch_gemm_tn(f->st, g));
  if (halves) HIPCHK(f, launch_add_rows(f->st, f->J, f->slabs, f->N, f->P, f->ld));
  if (*fused_chunks > 0) {
    // J^T f = sum of the per-tile-row pieces; |f|^2 from the residual column
    double *gvec = f->redbuf + f->npk;
    HIPCHK(f, launch_colsum_reduce(f->st, f->slabs, *fused_chunks, f->P, gvec));
    HIPCHK(f, launch_copy_strided(f->st, f->J + f->P, f->ld, f->r, 1, f->N, 1));
    HIPCHK(f, launch_sumsq(f->st, f->r, f->N, f->partial, gvec + f->P));
  }
  return 0;
}

// ---- the normal equations: J, J^T J (packed), J^T f, chi2 at device parameters p ------------------------------------------
// What one evaluation will run, decided up front from the handle and the call.
struct NormalRoute {
  // FUSED: few parameters, uncorrelated rows, a compiled formula -- J^T J, J^T f and chi2 straight from the model kernel's
  // registers (jit.hip lsqamd_jit_nrm), the Jacobian is never written, the evaluation reads x, y, w once.  Device-resident
  // LM only (the host-side drivers and the getters call ensure_J() when they need the rows).  LSQAMD_FUSED_NORMAL=0 disables.
  // SYNTH: the raw Jacobian rows are synthesised inside the whitening product (never written, never re-read).
  // GENERAL: the Jacobian is written, then whitened.
  enum Jac { FUSED, SYNTH, GENERAL } jac;
  int nq;             // FUSED: sums per workgroup of the fused kernel
  // the exchange in groups (sharded fits with the library's communicator): launch g forms the tile rows of
  // group g, its slab sum packs them, and their sum over the ranks runs on the exchange stream while launch g + 1 computes
  bool grouped;
  bool robust;        // rows rescaled by the loss before the products see them: the unfused routes
  bool with_prior;    // this rank adds the prior's share of J^T J, g and chi2
  bool defer_prior;   // ... its share of g and chi2 inside the caller's accept-tail kernel (one launch fewer)
  bool r_here;        // f->r already holds the whitened residual at p: the trial evaluation left it
  bool mirror;        // g, the column norms and chi2 go to the host (else the caller keeps them on the device: iterate_device)
};

static NormalRoute choose_route(const lsqamd_fit *f, bool mirror, bool r_here) {
  static const bool nrm_off = [] { const char *e = getenv("LSQAMD_FUSED_NORMAL"); return e && e[0] == '0'; }();
  const int64_t P = f->P;
  const int nbk = f->cfg.n_blocks;
  const int64_t B0 = nbk > 0 ? f->h_size[0] : 0;
  NormalRoute rt;
  rt.mirror = mirror;
  rt.r_here = r_here;
  rt.robust = f->robust();
  rt.with_prior = f->cfg.has_prior && f->adds_prior;
  rt.nq = (!mirror && !rt.robust && !nrm_off && f->nrm_part && f->progs.empty() && nbk == 0 && !f->have_param_rows && f->N > 0)
              ? lsqamd_jit::normal_nq(static_cast<const lsqamd_jit::Kernel *>(f->jit)) : 0;
  const bool synth = rt.nq == 0 && !rt.robust && nbk > 0 && f->uniform_blocks && f->uniform_tri && !f->have_param_rows &&
                     f->cfg.n_x <= 1 && f->h_row0[0] == 0 && (int64_t)nbk * B0 == f->N &&
                     whiten_synth_eligible(f->cfg.model, B0, P) &&
                     (int64_t)nbk * (B0 / 128) * P <= (int64_t)f->splits * P * f->ldm;
  rt.jac = rt.nq > 0 ? NormalRoute::FUSED : synth ? NormalRoute::SYNTH : NormalRoute::GENERAL;
  rt.grouped = rt.jac != NormalRoute::FUSED && f->comm && f->xg > 1 && P > 64 && f->N > 0;
  // (r_here: the trial evaluation at this point left Lambda (p - pbar) in tvec for the tail kernel)
  rt.defer_prior = rt.with_prior && r_here && !mirror && small_fuse(f);
  return rt;
}

// What an evaluation that keeps its results on the device (mirror == false) notes on the handle once everything is queued ...
static void note_device_eval(lsqamd_fit *f) {
  f->have_cov = false;
  f->have_dense_A = false;
  f->njev++;
  f->mirrors_stale = true;
}
// ... and what run_half restates after it has REPLAYED the accepted half step from a captured graph, in place of
// enqueue_accept's host side.  J_stale: the captured branch formed its normal equations with or without writing J -- a
// handle takes the FUSED route for all of its accepted steps or for none.  (nrm_in_tail and prior_deferred are the
// capture's own, and still on the handle.)
void note_accept_replayed(lsqamd_fit *f) {
  f->r_fresh = false;
  f->J_stale = f->used_nrm;
  note_device_eval(f);
}

// FUSED, the whole evaluation.  Flags: nrm_in_tail, J_stale, used_nrm, prior_deferred, then note_device_eval
static int normal_fused(lsqamd_fit *f, const double *p, const NormalRoute &rt) {
  const int64_t P = f->P;
  double *gv = f->redbuf + f->npk;
  {
    Scope sc(f, LSQAMD_T_JACOBIAN);
    int64_t blocks = (f->N + 255) / 256;
    if (blocks > NRM_BLOCKS) blocks = NRM_BLOCKS;
    lsqamd_jit::LaunchArgs la;
    la.x = f->x; la.p = p; la.ymean = f->ymean; la.wdiag = f->wdiag; la.n_data = f->N;
    HIPCHK(f, lsqamd_jit::launch_normal(static_cast<const lsqamd_jit::Kernel *>(f->jit), f->st, la, f->nrm_part, (int)blocks));
    // few rows as well, one rank: totalling the sums and unpacking them is left to the accept-tail kernel (one launch
    // instead of three); the prior's share of g and chi2 then has to be deferred to it too
    f->nrm_in_tail = blocks <= 64 && small_fuse(f) && (!rt.with_prior || rt.r_here) ? (int)blocks : 0;
    if (!f->nrm_in_tail) {
      double *tot = f->nrm_part + (int64_t)NRM_BLOCKS * 96;
      HIPCHK(f, launch_colsum_reduce(f->st, f->nrm_part, blocks, rt.nq, tot));
      HIPCHK(f, launch_nrm_unpack(f->st, tot, P, f->redbuf, gv, rt.with_prior ? f->prior_prec : nullptr, f->cfg.prior_dense));
    }
  }
  f->J_stale = true;
  f->used_nrm = true;
  {
    Scope sc(f, LSQAMD_T_GRAD);
    f->prior_deferred = rt.defer_prior;
    if (rt.with_prior && !rt.defer_prior)
      HIPCHK(f, launch_add_prior(f->st, f->redbuf, P, f->prior_prec, f->cfg.prior_dense, f->prior_mean, p, f->tvec, gv, 0,
                                 rt.r_here ? 1 : 0));
  }
  const int rc = do_reduce(f, f->redbuf, f->npk + P + 1);
  if (rc) return rc;
  note_device_eval(f);
  return 0;
}

// SYNTH: the whitened residual -- column P, and the weights of the fused J^T f -- is the one the trial evaluation just left
// in f->r when this IS the trial point, else it is evaluated here; J^T f and |f|^2 come out of the product.  Flag: used_synth
static int jacobian_synth(lsqamd_fit *f, const double *p, const NormalRoute &rt, int64_t *fused_chunks) {
  const int64_t P = f->P, B0 = f->h_size[0];
  const int nbk = f->cfg.n_blocks;
  {
    Scope sc(f, LSQAMD_T_JACOBIAN);
    if (!rt.r_here) {
      const int rc = residual_vector_launch(f, p);
      if (rc) return rc;
    }
    HIPCHK(f, launch_copy_strided(f->st, f->r, 1, f->J + P, f->ld, f->N, 1));
  }
  Scope sc(f, LSQAMD_T_WHITEN);
  WhitenSynth w;
  w.model = f->cfg.model; w.Wt = f->wt; w.x = f->x; w.p = p; w.J = f->J; w.ld = f->ld;
  w.B = B0; w.K = P / 2; w.nb = nbk; w.colsum_out = f->slabs;
  w.trig_far = (f->cfg.model == LSQAMD_MODEL_COSMIX && f->have_x && trig_split_pays(f)) ? f->trig_far : nullptr;   // current: set with the residual at p
  HIPCHK(f, launch_whiten_synth(f->st, w));
  f->used_synth = true;
  *fused_chunks = (int64_t)nbk * (B0 / 128);
  double *gv = f->redbuf + f->npk;
  HIPCHK(f, launch_colsum_reduce(f->st, f->slabs, *fused_chunks, P, gv));
  HIPCHK(f, launch_sumsq(f->st, f->r, f->N, f->partial, gv + P));
  return 0;
}

// GENERAL: the Jacobian written by the model kernel, whitened, rescaled by the loss of a robust fit
static int jacobian_general(lsqamd_fit *f, const double *p, const NormalRoute &rt, int64_t *fused_chunks) {
  const int64_t P = f->P;
  {
    Scope sc(f, LSQAMD_T_JACOBIAN);
    ModelArgs m = model_args(f, p);
    HIPCHK(f, launch_jacobian_ex(f->st, m, f->J, f->Jraw, f->ld));
    if (f->have_param_rows)
      HIPCHK(f, launch_param_rows(f->st, f->row_param, f->N, f->P, f->ld, p, f->ymean, f->wdiag,
                                  f->cfg.n_blocks > 0 ? f->in_block : nullptr, f->J, f->Jraw, 1));
  }
  const int rc = whiten_jacobian(f, fused_chunks, rt.r_here, rt.robust);
  if (rc) return rc;
  if (rt.robust) {
    // scipy's scale_for_robust_loss_function on the whitened rows [J | f] (robust.hip); the cost of this point
    // (red_scalar[2], put in chi2's place once J^T f has been formed) from the residual column before it is rescaled
    HIPCHK(f, launch_robust_cost(f->st, f->J + P, f->N, f->ld, f->loss, f->f_scale, f->partial, f->red_scalar + 2));
    HIPCHK(f, launch_robust_scale_rows(f->st, f->J, f->N, P, f->ld, f->loss, f->f_scale));
  }
  return 0;
}

// J^T f, chi2 (+ the prior's share) into gvec: after the LAST product launch.  syrk_colsum: that launch left them in
// f->partial; else, unless the whitening product formed them already (fused_chunks > 0), one more pass over J.
// Flag: prior_deferred
static int finish_gvec(lsqamd_fit *f, const double *p, const NormalRoute &rt, int64_t fused_chunks, bool syrk_colsum) {
  const int64_t P = f->P;
  double *gvec = f->redbuf + f->npk;
  if (syrk_colsum)
    HIPCHK(f, launch_colsum_reduce(f->st, f->partial, f->splits, P + 1, gvec));
  else if (fused_chunks == 0)
    HIPCHK(f, launch_colsum_dot(f->st, f->J, f->N, f->ld, P + 1, P, f->partial, f->npartial, gvec));
  if (rt.robust) HIPCHK(f, launch_copy_strided(f->st, f->red_scalar + 2, 1, gvec + P, 1, 1, 1));   // 2 x cost, not |f_scaled|^2
  f->prior_deferred = rt.defer_prior;
  if (rt.with_prior && !rt.defer_prior)
    HIPCHK(f, launch_add_prior(f->st, f->redbuf, P, f->prior_prec, f->cfg.prior_dense,
                               f->prior_mean, p, f->tvec, gvec, 0, rt.r_here ? 1 : 0));
  return 0;
}

// the slab sum and the prior precision in ONE pass over the packed tiles [tile0, tile0 + n_tiles) (-1: all of them), on `on`
// (when splits == 1 the kernel ignored split_stride and wrote slab 0 directly)
static int pack_tiles(lsqamd_fit *f, const NormalRoute &rt, hipStream_t on, int64_t tile0, int64_t n_tiles) {
  HIPCHK(f, launch_finalize_pack(on, f->slabs, f->splits, f->P * f->ldm, f->P, f->ldm, f->redbuf,
                                 rt.with_prior ? f->prior_prec : nullptr, f->cfg.prior_dense, tile0, n_tiles));
  return 0;
}

// group q of the packed matrix summed over the ranks on the exchange stream, "done" recorded behind it
static int exchange_group(lsqamd_fit *f, int q) {
  {
    Scope sc(f, LSQAMD_T_EXCH_COLL, f->xst);
    const int64_t off = f->xg_tile[q] * 128 * 128;
    const int64_t cnt = (q == f->xg - 1 ? f->npk + f->P + 1 : f->xg_tile[q + 1] * 128 * 128) - off;   // the last group carries [J^T f | chi2]
    const int rc = comm_all_reduce_on(f, f->xst, f->redbuf + off, cnt);
    if (rc) return rc;
  }
  HIPCHK(f, hipEventRecord(f->xg_done[q], f->xst));
  return 0;
}

// The product in exchange groups.  Signal form: ONE product launch; the exchange stream follows it group by group through the
// counters.  Split form: one product launch per group, each followed by its pack on the step's stream.
static int product_grouped(lsqamd_fit *f, const double *p, const NormalRoute &rt, const GemmTN &g, int64_t fused_chunks,
                           bool syrk_colsum) {
  // developer knob LSQAMD_EXCHANGE_DEBUG: 's' nothing on the exchange stream before the product is done; 'n' that, and the
  // grouped ORDER with the plain kernel (no counters, no waits for them)
  static const int dbg = [] { const char *e = getenv("LSQAMD_EXCHANGE_DEBUG"); return e ? (e[0] == 's' ? 1 : (e[0] == 'n' ? 2 : 0)) : 0; }();
  int rc = 0;
  if (!f->xst) f->xst = stream_take();
  for (int q = 0; q < f->xg; ++q) {
    if (!f->xg_ready[q]) f->xg_ready[q] = event_take();
    if (!f->xg_done[q]) f->xg_done[q] = event_take();
  }
  if (!f->xst) FAIL(f, LSQAMD_EHIP, "no stream for the grouped exchange");
  if (f->xg_signal) {
    HIPCHK(f, hipMemsetAsync(f->xg_ctr, 0, 8 * sizeof(int32_t), f->st));
    HIPCHK(f, hipEventRecord(f->xg_ready[0], f->st));          // "the counters are zero": nothing on xst reads them earlier
    HIPCHK(f, hipStreamWaitEvent(f->xst, f->xg_ready[0], 0));
    {
      Scope sc(f, LSQAMD_T_SYRK);
      GemmTN gq = g;
      gq.work_map = f->syrk_map_g;
      gq.n_work = f->syrk_nwork;
      gq.done_ctr = dbg == 2 ? nullptr : f->xg_ctr;
      HIPCHK(f, launch_gemm_tn(f->st, gq));
    }
    {
      Scope sc(f, LSQAMD_T_GRAD);
      if ((rc = finish_gvec(f, p, rt, fused_chunks, syrk_colsum))) return rc;
    }
    HIPCHK(f, hipEventRecord(f->xg_ready[1], f->st));          // "[J^T f | chi2] is final" (goes out with the last group)
    if (dbg) HIPCHK(f, hipStreamWaitEvent(f->xst, f->xg_ready[1], 0));
    for (int q = 0; q < f->xg; ++q) {
      if (dbg != 2) HIPCHK(f, launch_wait_counter(f->xst, f->xg_ctr + q, f->xg_count[q], f->xg_ctr + 8));
      {
        Scope sc(f, LSQAMD_T_GRAD, f->xst);
        if ((rc = pack_tiles(f, rt, f->xst, f->xg_tile[q], f->xg_tile[q + 1] - f->xg_tile[q]))) return rc;
      }
      if (q == f->xg - 1) HIPCHK(f, hipStreamWaitEvent(f->xst, f->xg_ready[1], 0));
      if ((rc = exchange_group(f, q))) return rc;
    }
  } else {
    for (int q = 0; q < f->xg; ++q) {
      {
        Scope sc(f, LSQAMD_T_SYRK);
        GemmTN gq = g;
        gq.work_map = f->syrk_map_g + 4 * (int64_t)f->xg_work[q];
        gq.n_work = f->xg_work[q + 1] - f->xg_work[q];
        HIPCHK(f, launch_gemm_tn(f->st, gq));
      }
      {
        Scope sc(f, LSQAMD_T_GRAD);
        if ((rc = pack_tiles(f, rt, f->st, f->xg_tile[q], f->xg_tile[q + 1] - f->xg_tile[q]))) return rc;
        if (q == f->xg - 1 && (rc = finish_gvec(f, p, rt, fused_chunks, syrk_colsum))) return rc;
      }
      HIPCHK(f, hipEventRecord(f->xg_ready[q], f->st));
      HIPCHK(f, hipStreamWaitEvent(f->xst, f->xg_ready[q], 0));
      if ((rc = exchange_group(f, q))) return rc;
    }
  }
  Scope sc(f, LSQAMD_T_REDUCE);
  Scope sc2(f, LSQAMD_T_EXCH_WAIT);
  for (int q = 0; q < f->xg; ++q) HIPCHK(f, hipStreamWaitEvent(f->st, f->xg_done[q], 0));
  return 0;
}

// J^T J into the slabs (split-K, upper tiles), packed with the prior precision into f->redbuf; [J^T f | chi2] behind it; the
// sum of all of it over the ranks
static int product_and_exchange(lsqamd_fit *f, const double *p, const NormalRoute &rt, int64_t fused_chunks) {
  const int64_t P = f->P;
  GemmTN g;
  g.X = f->J; g.Y = f->J; g.ldx = g.ldy = f->ld;
  g.C = f->slabs; g.ldc = f->ldm;
  g.M = P; g.N = P; g.K = f->N;
  g.upper_only = 1;
  g.splits = f->splits;
  g.split_stride = P * f->ldm;
  if (P > 64) {   // (one tile: nothing to order, and the 64 x 64 kernel takes no work list)
    g.work_map = f->syrk_map;
    g.n_work = f->syrk_nwork;
  }
  bool syrk_colsum = false;
  if (fused_chunks == 0 && f->N > 0) {   // J^T f and chi2 out of the diagonal tiles of this launch, when it is that kernel
    g.colsum_out = f->partial;            // [splits][P + 1] (splits <= 256 <= npartial)
    g.colsum_ld = P + 1;
    g.colsum_rcol = P;
    if (gemm_tn_fuses_colsum(g)) syrk_colsum = true;
    else g.colsum_out = nullptr;
  }
  if (rt.grouped) return product_grouped(f, p, rt, g, fused_chunks, syrk_colsum);
  {
    Scope sc(f, LSQAMD_T_SYRK);
    if (f->N > 0) {
      HIPCHK(f, launch_gemm_tn(f->st, g));
    } else {
      HIPCHK(f, hipMemsetAsync(f->slabs, 0, sizeof(double) * f->splits * P * f->ldm, f->st));
    }
  }
  {
    Scope sc(f, LSQAMD_T_GRAD);
    int rc = pack_tiles(f, rt, f->st, 0, -1);
    if (rc || (rc = finish_gvec(f, p, rt, fused_chunks, syrk_colsum))) return rc;
  }
  return do_reduce(f, f->redbuf, f->npk + P + 1);
}

// g, the column norms and chi2 to the host (one synchronisation).  Flags: have_cov, have_dense_A, njev
static int mirror_to_host(lsqamd_fit *f) {
  const int64_t P = f->P;
  f->have_cov = false;
  f->have_dense_A = false;
  HIPCHK(f, hipMemcpyAsync(f->pin_g, f->redbuf + f->npk, sizeof(double) * (P + 1), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(f->pin_c, f->diag_dev, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  for (int64_t j = 0; j < P; ++j) {
    f->hg[j] = f->pin_g[j];
    f->hcoln[j] = std::sqrt(f->pin_c[j] > 0.0 ? f->pin_c[j] : 0.0);
  }
  f->chi2 = f->pin_g[P];
  f->njev++;
  if (!std::isfinite(f->chi2)) FAIL(f, LSQAMD_ENONFINITE, "chi2 is not finite at this point");
  return 0;
}

// J, J^T J (packed), J^T f, chi2 at device parameters p; host g/chi2/colnorm refreshed (mirror) or left to the caller's
// accept-tail kernel.  Flags of the unfused routes: J_stale, nrm_in_tail, cov_unavailable here; the rest in the stages
int eval_normal_dev(lsqamd_fit *f, const double *p, bool mirror) {
  const bool r_here = f->r_fresh && f->r_ptr == p;
  f->r_fresh = false;
  const NormalRoute rt = choose_route(f, mirror, r_here);
  if (rt.jac == NormalRoute::FUSED) return normal_fused(f, p, rt);
  f->J_stale = false;
  f->nrm_in_tail = 0;
  f->cov_unavailable = false;
  int64_t fused_chunks = 0;
  int rc = rt.jac == NormalRoute::SYNTH ? jacobian_synth(f, p, rt, &fused_chunks) : jacobian_general(f, p, rt, &fused_chunks);
  if (rc) return rc;
  if ((rc = product_and_exchange(f, p, rt, fused_chunks))) return rc;
  if (!mirror) {   // (the column norms: lm_accept_tail_kernel, the caller's next launch)
    note_device_eval(f);
    return 0;
  }
  HIPCHK(f, launch_packed_diag(f->st, f->redbuf, f->P, f->diag_dev));
  return mirror_to_host(f);
}

// (A + mu D^2) v = g  -> f->hv ; returns LSQAMD_ENOTPD when a pivot fails
// launches only: factor (A + mu D^2 | g) and back-substitute; v lands in f->yv[P..2P).
// diag_host == nullptr: D is the device-resident mirror (no host-to-device copy: on this platform
// an SDMA upload followed by a dependent kernel costs ~100 us of cross-engine synchronisation)
// frozen_host (with mu = 0, dogbox): flags of the parameters taken out of the system
int solve_damped_launch(lsqamd_fit *f, double mu, const double *diag_host, const double *frozen_host, bool fetch,
                        const double *mu_dev, bool factor_only) {
  const int64_t P = f->P;
  double *gvec = f->redbuf + f->npk;
  {
    Scope sc(f, LSQAMD_T_CHOLESKY);
    const double *dd = f->dscale, *frozen = nullptr;
    if (diag_host || frozen_host) {
      std::memcpy(f->pin_d, diag_host ? diag_host : frozen_host, sizeof(double) * P);
      HIPCHK(f, hipMemcpyAsync(f->diag_dev, f->pin_d, sizeof(double) * P, hipMemcpyHostToDevice, f->st));
      if (diag_host) dd = f->diag_dev;
      else frozen = f->diag_dev;
    }
    // (the pivot-failure word is cleared by the kernel that builds the matrix, the hand-off granules of the
    // back substitution by the one that copies its right-hand side: two memsets fewer per trial)
    HIPCHK(f, launch_build_damped(f->st, f->redbuf, P, f->ldm, mu, dd, gvec, f->M, frozen, mu_dev, f->info_dev));
    HIPCHK(f, potrf_upper(f->st, f->M, P, f->ldm, f->ncols_aug, f->chol_work, f->info_dev, true));
  }
  if (factor_only) return 0;    // (small systems: the caller's single-workgroup kernel does the rest)
  {
    Scope sc(f, LSQAMD_T_SOLVE);
    HIPCHK(f, launch_copy_column_zero(f->st, f->M + P, f->ldm, f->yv, P, f->yv + 2 * P, backsolve_scratch_bytes(P)));
    HIPCHK(f, backsolve_upper(f->st, f->M, P, f->ldm, f->chol_work, f->yv, f->yv + 2 * P, f->info_dev, true));
    if (fetch) {
      HIPCHK(f, hipMemcpyAsync(f->pin_v, f->yv + P, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
      HIPCHK(f, hipMemcpyAsync(f->pin_s + 4, f->info_dev, sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    }
  }
  return 0;
}

// after the stream has been synchronised: v -> f->hv; LSQAMD_ENOTPD when a pivot failed
int solve_damped_collect(lsqamd_fit *f) {
  const int64_t P = f->P;
  int32_t info = 0;
  std::memcpy(f->hv.data(), f->pin_v, sizeof(double) * P);
  std::memcpy(&info, f->pin_s + 4, sizeof(int32_t));
  f->ntrial++;
  if (info == -77) FAIL(f, LSQAMD_EHIP, "back substitution: a workgroup of the chain gave up waiting");
  if (info != 0) {
    f->chol_fail++;
    return LSQAMD_ENOTPD;
  }
  for (int64_t j = 0; j < P; ++j)
    if (!std::isfinite(f->hv[j])) {
      f->chol_fail++;
      return LSQAMD_ENOTPD;
    }
  return 0;
}

// (A + mu D^2) v = g  -> f->hv ; returns LSQAMD_ENOTPD when a pivot fails
int solve_damped_dev(lsqamd_fit *f, double mu, const double *diag_host, const double *frozen_host) {
  const int rc = solve_damped_launch(f, mu, diag_host, frozen_host);
  if (rc) return rc;
  HIPCHK(f, hipStreamSynchronize(f->st));
  return solve_damped_collect(f);
}

void scale_init(lsqamd_fit *f) {
  (void)launch_scale_update(f->st, f->P, f->opt.scaler, 1, f->diag_dev, f->dscale);  // diag_dev = coln^2
  for (int64_t j = 0; j < f->P; ++j) {
    if (f->opt.scaler == LSQAMD_SCALE_LEVENBERG)    // (scipy methods: D = 1 / x_scale, lsqamd_set_x_scale)
      f->hdiag[j] = (f->opt.trs >= LSQAMD_TRS_TRF && !f->x_scale.empty()) ? 1.0 / f->x_scale[j] : 1.0;
    else f->hdiag[j] = f->hcoln[j] == 0.0 ? 1.0 : f->hcoln[j];
  }
}

void scale_update(lsqamd_fit *f) {
  (void)launch_scale_update(f->st, f->P, f->opt.scaler, 0, f->diag_dev, f->dscale);
  for (int64_t j = 0; j < f->P; ++j) {
    if (f->opt.scaler == LSQAMD_SCALE_MORE) f->hdiag[j] = std::fmax(f->hdiag[j], f->hcoln[j]);
    else if (f->opt.scaler == LSQAMD_SCALE_MARQUARDT) f->hdiag[j] = f->hcoln[j] == 0.0 ? 1.0 : f->hcoln[j];
  }
}

// ---- pieces shared by the trust-region sub-problem solvers -------------------
// y = A x with A = the reduced J^T J (+ prior): dense symmetric copy kept in f->Wl
int symv_host(lsqamd_fit *f, const double *x, double *y) {
  const int64_t P = f->P;
  if (!f->have_dense_A) {
    HIPCHK(f, launch_unpack_sym(f->st, f->redbuf, P, f->Wl, f->ldm));
    f->have_dense_A = true;
  }
  HIPCHK(f, hipMemcpyAsync(f->tvec, x, sizeof(double) * P, hipMemcpyHostToDevice, f->st));
  HIPCHK(f, launch_gemv_rows(f->st, f->Wl, f->ldm, P, P, f->tvec, f->yv));
  HIPCHK(f, hipMemcpyAsync(y, f->yv, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
}

double dot_h(const std::vector<double> &a, const std::vector<double> &b) {
  double s = 0.0;
  for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
  return s;
}

// (A + mu D^2) out = rhs with the factor U already in f->M (lmaccel's second solve, lm.c lm_step):
// forward substitution block by block through the TN GEMM (X = inv(U_kk), then X = U[k, k+1:]),
// then the usual back substitution.
int solve_with_factor(lsqamd_fit *f, const double *rhs, double *out) {
  const int64_t P = f->P;
  HIPCHK(f, hipMemcpyAsync(f->yv, rhs, sizeof(double) * P, hipMemcpyHostToDevice, f->st));
  for (int64_t k0 = 0; k0 < P; k0 += 128) {
    const int64_t nb = P - k0 < 128 ? P - k0 : 128;
    GemmTN a;  // y_k <- inv(U_kk)^T y_k
    a.X = f->chol_work + (k0 / 128) * 128 * 128; a.ldx = 128;
    a.Y = f->yv + k0; a.ldy = 1; a.C = f->yv + k0; a.ldc = 1;
    a.M = nb; a.N = 1; a.K = nb;
    a.x_upper_tri = 1;
    HIPCHK(f, launch_gemm_tn(f->st, a));
    const int64_t rest = P - (k0 + nb);
    if (rest <= 0) continue;
    GemmTN b;  // y_rest -= U[k, rest]^T y_k
    b.X = f->M + k0 * f->ldm + k0 + nb; b.ldx = f->ldm;
    b.Y = f->yv + k0; b.ldy = 1; b.C = f->yv + k0 + nb; b.ldc = 1;
    b.M = rest; b.N = 1; b.K = nb;
    b.alpha = -1.0; b.beta = 1.0;
    HIPCHK(f, launch_gemm_tn(f->st, b));
  }
  HIPCHK(f, backsolve_upper(f->st, f->M, P, f->ldm, f->chol_work, f->yv, f->yv + 2 * P, f->info_dev));
  HIPCHK(f, hipMemcpyAsync(out, f->yv + P, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
}

// G_h = J(x)^T r(x_h) + Lambda (x_h - pbar): the gradient-like vector the finite-difference
// second directional derivative needs (fdfvv.c), all-reduced like the gradient
int grad_like_at(lsqamd_fit *f, const double *xh, double *out) {
  const int64_t P = f->P;
  HIPCHK(f, hipMemcpyAsync(f->p_trial, xh, sizeof(double) * P, hipMemcpyHostToDevice, f->st));
  double c2 = 0.0;
  int rc = eval_residual_dev(f, f->p_trial, &c2);  // f->r = whitened residual at x_h
  if (rc) return rc;
  if ((rc = ensure_J(f))) return rc;
  HIPCHK(f, launch_colsum_dot(f->st, f->J, f->N, f->ld, P, P, f->partial, f->npartial, f->yv, f->r));
  if (f->cfg.has_prior && f->adds_prior)
    HIPCHK(f, launch_add_prior(f->st, nullptr, P, f->prior_prec, f->cfg.prior_dense, f->prior_mean,
                               f->p_trial, f->tvec, f->yv, 0));
  rc = do_reduce(f, f->yv, P);
  if (rc) return rc;
  HIPCHK(f, hipMemcpyAsync(out, f->yv, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
}

// the whitened Jacobian at the current point in f->J, written now if the last normal equations were formed without it
int ensure_J(lsqamd_fit *f) {
  if (!f->J_stale) return 0;
  ModelArgs m = model_args(f, f->p_dev);
  HIPCHK(f, launch_jacobian_ex(f->st, m, f->J, f->Jraw, f->ld));
  if (f->cfg.n_blocks > 0) {   // (the one-launch fit kernel takes correlated rows too: their whitening product is redone here)
    int64_t fused = 0;
    const int rc = whiten_jacobian(f, &fused, false);
    if (rc) return rc;
  }
  f->J_stale = false;
  return 0;
}

// host copies of x, g, D, the column norms and the last step after iterations that kept them on
// the device
int refresh_mirrors(lsqamd_fit *f) {
  if (!f->mirrors_stale) return 0;
  const int64_t P = f->P;
  HIPCHK(f, hipMemcpyAsync(f->pin_x, f->p_dev, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(f->pin_g, f->redbuf + f->npk, sizeof(double) * (P + 1), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(f->pin_d, f->dscale, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(f->pin_c, f->diag_dev, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(f->pin_v, f->yv + P, sizeof(double) * P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  for (int64_t j = 0; j < P; ++j) {
    f->hx[j] = f->pin_x[j];
    f->hg[j] = f->pin_g[j];
    f->hdiag[j] = f->pin_d[j];
    f->hcoln[j] = std::sqrt(f->pin_c[j] > 0.0 ? f->pin_c[j] : 0.0);
    f->hv[j] = f->pin_v[j];
    f->hdx[j] = -f->pin_v[j];
  }
  f->mirrors_stale = false;
  return 0;
}

// f->logdet = log det of the normal matrix in f->redbuf (NaN when it has no Cholesky factor); f->cov is left alone
int logdet_normal(lsqamd_fit *f) {
  const int64_t P = f->P;
  int32_t info = 0;
  double ld = 0.0;
  HIPCHK(f, launch_build_damped(f->st, f->redbuf, P, f->ldm, 0.0, f->diag_dev, nullptr, f->M));
  HIPCHK(f, potrf_upper(f->st, f->M, P, f->ldm, P, f->chol_work, f->info_dev));
  HIPCHK(f, logdiag_sum(f->st, f->M, P, f->ldm, f->scal));
  HIPCHK(f, hipMemcpyAsync(&info, f->info_dev, sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(&ld, f->scal, sizeof(double), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  f->logdet = info != 0 ? NAN : 2.0 * ld;
  return info != 0 ? LSQAMD_ENOTPD : 0;
}

// covariance + logdet at the current point: factor A (mu = 0), invert
static int do_covariance_chol(lsqamd_fit *f);
int do_covariance(lsqamd_fit *f) {
  f->cov_host_valid = false;
  f->cov_inaccurate = false;
  f->cov_dropped = 0;
  const int rc = f->opt.solver == LSQAMD_SOLVER_QR ? do_covariance_qr(f) : do_covariance_chol(f);
  if (rc == LSQAMD_ENOTPD) {
    // a rank-deficient final Jacobian: the reference's plugins return a truncated inverse there (rankdef.hip)
    const std::string keep = f->err;
    const int k = covariance_rank_deficient(f);
    if (k > 0) {
      f->cov_dropped = k;
      return 0;
    }
    f->err = keep;
  }
  return rc;
}

static int do_covariance_chol(lsqamd_fit *f) {
  const int64_t P = f->P;
  Scope sc(f, LSQAMD_T_COVAR);
  int32_t info = 0;
  double ld = 0.0;
  HIPCHK(f, launch_build_damped(f->st, f->redbuf, P, f->ldm, 0.0, f->diag_dev, nullptr, f->M));
  HIPCHK(f, potrf_upper(f->st, f->M, P, f->ldm, P, f->chol_work, f->info_dev));
  HIPCHK(f, logdiag_sum(f->st, f->M, P, f->ldm, f->scal));
  f->have_dense_A = false;  // Wl is reused below
  HIPCHK(f, trtri_upper_to_lower_T(f->st, f->M, P, f->ldm, f->chol_work, f->Wl, f->ldm));
  GemmTN g;
  g.X = f->Wl; g.Y = f->Wl; g.ldx = g.ldy = f->ldm;
  g.C = f->cov; g.ldc = f->ldm;
  g.M = P; g.N = P; g.K = P;
  g.upper_only = 1;
  g.xy_lower_tri = 1;
  HIPCHK(f, launch_gemm_tn(f->st, g));
  HIPCHK(f, launch_symmetrize_from_upper(f->st, f->cov, P, f->ldm));
  HIPCHK(f, hipMemcpyAsync(&info, f->info_dev, sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(&ld, f->scal, sizeof(double), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  f->have_cov = true;
  if (info != 0) {
    f->logdet = NAN;
    char b[160];
    snprintf(b, sizeof(b), "J^T J is not positive definite at the solution (pivot %d); covariance undefined", info);
    f->err = b;
    return LSQAMD_ENOTPD;
  }
  f->logdet = 2.0 * ld;
  return 0;
}

}  // namespace lsqamd_host
