// Internal to the host side of the single-fit library: what pool.hip, workspace.hip, eval.hip, lm_driver.hip and api.hip
// share besides the handle itself (fit_state.h, which qr.hip, rankdef.hip and comm.hip see too; scipy_methods.hip: DBL_EPS).
// One-line predicates of the hot host path are inline here: a half step of a small fit is ~27 us, and none of them may
// turn into a call across translation units.  Not part of the C ABI.
#pragma once
#include <atomic>

#include "fit_state.h"

namespace lsqamd_host {

constexpr int64_t ALIGN = 256;
constexpr int NRM_BLOCKS = 1024;   // workgroups of the fused normal-equation kernel (few parameters, jit.hip)
constexpr double DBL_EPS = 2.220446049250313e-16;   // machine epsilon (GSL_DBL_EPSILON, numpy's finfo(float).eps, MINPACK's epsmch)
inline int64_t rup(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct Carver {   // hands out 256-byte aligned pieces of one device block (dry: only adds the sizes up)
  char *base;
  size_t off = 0, cap;
  bool dry;
  Carver(void *b, size_t c, bool d) : base((char *)b), cap(c), dry(d) {}
  template <typename T>
  T *take(int64_t count) {
    const size_t bytes = (size_t)rup((int64_t)(count < 1 ? 1 : count) * (int64_t)sizeof(T), ALIGN);
    T *p = dry ? nullptr : reinterpret_cast<T *>(base + off);
    off += bytes;
    return p;
  }
};

// small single-rank fits: fused single-workgroup tails (LSQAMD_SMALL_FUSE=0: the general kernels)
inline bool small_fuse(const lsqamd_fit *f) {
  const char *e = getenv("LSQAMD_SMALL_FUSE");     // read per call (tests flip it between fits; a getenv is ~50 ns)
  return !(e && e[0] == '0') && !f->comm && !f->reduce;
}

// two extra launches per evaluation (the range kernel and the variant that finds nothing to do, ~5 us together)
// buy a trig kernel without far-range code: worth it from a few million cosines per evaluation on
inline bool trig_split_pays(const lsqamd_fit *f) { return f->N * (f->P / 2) >= ((int64_t)1 << 22); }

// ---- pool.hip: process-wide recycling (declared in fit_state.h), hand-off counters, test poison, event timers --------------
int current_device();   // -1: the runtime could not say
extern std::atomic<int64_t> g_handoff[3];   // not verified (yet) / served from device memory / differed from the device's copy
bool poison_pinned();   // LSQAMD_POISON_PINNED=1, read once per process
void poison_fill(void *p, size_t bytes);
void resolve_timers(lsqamd_fit *f, bool only_if_many = false);

// ---- workspace.hip: sizing and carving of the caller's workspace, what a handle must have been given before it runs -------
size_t carve(lsqamd_fit *f, void *ws, size_t cap, bool dry);
int check_cfg(const lsqamd_config *c);
lsqamd::ModelArgs model_args(const lsqamd_fit *f, const double *p);
int device_ok(lsqamd_fit *f);
int ready(lsqamd_fit *f);
// the exchange groups of a sharded fit (LSQAMD_EXCHANGE_GROUPS, read here): f->xg*, and for more than one group their work
// list in wm[4 * f->syrk_nwork] -- the caller uploads it to f->syrk_map_g.  0 or LSQAMD_EHIP
int plan_exchange_groups(lsqamd_fit *f, int32_t *wm);

// ---- eval.hip: the evaluation blocks (more of them in fit_state.h) ---------------------------------------------------
// whitened residual at device parameters p -> f->r; chi2 (summed over ranks) -> f->red_scalar[0].  Launches only.
// decide: a single rank's trial -- the sum of squares' second stage, the prior's share and the LM decision in one launch
int eval_residual_launch(lsqamd_fit *f, const double *p, bool decide = false);
// launches only: factor (A + mu D^2 | g) and back-substitute; v lands in f->yv[P..2P) (details at the definition)
int solve_damped_launch(lsqamd_fit *f, double mu, const double *diag_host, const double *frozen_host = nullptr,
                        bool fetch = true, const double *mu_dev = nullptr, bool factor_only = false);
int solve_damped_collect(lsqamd_fit *f);   // after the stream has been synchronised: v -> f->hv; LSQAMD_ENOTPD
void scale_init(lsqamd_fit *f);
int grad_like_at(lsqamd_fit *f, const double *xh, double *out);
int logdet_normal(lsqamd_fit *f);
// the host side of an accepted half step that was replayed from a captured graph (run_half): what eval_normal_dev(mirror =
// false) notes on the handle besides launching
void note_accept_replayed(lsqamd_fit *f);

// ---- lm_driver.hip -------------------------------------------------------------------------------------------------
int iterate(lsqamd_fit *f);             // one trust_iterate: 0 or LSQAMD_ENOPROG; negative on backend failure
int convergence_test(lsqamd_fit *f);
// iterate, nit, convergence test -> 0 and *info; an iteration without progress -> LSQAMD_ENOPROG (*info too) when stall_ends
int driver_iteration(lsqamd_fit *f, int *info, bool stall_ends);
void fill_summary(lsqamd_fit *f, lsqamd_summary *s, int status, int info);
// The two ways a GSL-method fit runs from p0; *status / *info: what lsqamd_run reports (fill_summary).
// A whole small fit in ONE launch -> 1: done; 0: not this fit's route (the general path runs it); < 0: error
int run_one_launch(lsqamd_fit *f, const double *p0, int *status, int *info);
int run_gsl_driver(lsqamd_fit *f, const double *p0, int *status, int *info);   // do_init + the driver loop: 0 or an error

}  // namespace lsqamd_host
