// What the kernels of the batched engine share (batch.hip: plain LM and the engine's host side; batch_trs.hip: the
// dogleg family): the packed-tile addressing, the workgroup reductions, the per-fit device scalars.
#pragma once
#include "common.h"

namespace lsqamd {

constexpr int TBK = 128;  // packed tile edge (vecops.hip)

__device__ __forceinline__ double bsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__device__ __forceinline__ double block_sum(double v, double *sh) {
  v = bsum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__device__ __forceinline__ double block_max(double v, double *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

__device__ __forceinline__ int64_t pk_diag(int64_t j, int64_t T) {  // packed offset of A[j][j]
  const int64_t tm = j / TBK, r = j % TBK;
  return (tm * T - tm * (tm - 1) / 2) * TBK * TBK + r * TBK + r;
}

struct BState {  // per-fit device scalars
  double *mu, *chi2, *chi2t, *vg, *dv2;
  int32_t *nu, *bad, *iter, *nit, *info, *status, *active, *accepted, *enoprog, *cholinfo, *nfev, *njev;
  int32_t *n_active;
  int32_t *moved;   // active and accepted this round: the only fits whose normal equations change
};

// ---- the dogleg family (LSQAMD_TRS_DOGLEG / DDOGLEG / SUBSPACE2D; batch_trs.hip) ------------------------
// per-fit record of TR_COUNT doubles: the trust radius, the predicted reduction of the trial step, and what the two legs
// of the current iterate reduce to (lm_driver.hip struct Legs)
enum {
  TR_DELTA = 0,   // trust radius
  TR_PRED = 1,    // -(dx^T A dx + 2 g.dx) of the trial step
  TR_NINVG = 2,   // |D^-1 g|
  TR_WAW = 3,     // w^T A w = |J D^-2 g|^2, w = D^-2 g
  TR_NSD = 4,     // |D dx_sd|
  TR_NGN = 5,     // |D dx_gn|
  TR_GSD = 6,     // g.dx_sd
  TR_GGN = 7,     // g.dx_gn
  TR_T = 8,       // ddogleg: the Gauss-Newton leg is shortened to t dx_gn (dogleg: 1)
  TR_BA = 9,      // dogleg_beta: a = |D (t dx_gn - dx_sd)|^2
  TR_BB = 10,     //              b = 2 (D dx_sd).(D (t dx_gn - dx_sd))
  TR_SC = 11,     // subspace2D: c = q0.q1 of the normalised legs
  TR_SR = 12,     //             r = |q1 - c q0| (rank test)
  TR_COUNT = 16
};

struct BTrs {
  double *rec;                      // [B][TR_COUNT]
  double *w, *aw, *dx_sd, *dx_gn;   // [B][P]
  double *part;                     // [B][T][T][TBK]: per-tile partial vectors of the symmetric product
  int32_t *gn_failed;               // no Gauss-Newton point at this iterate (J^T J has no Cholesky factor): gradient leg only
  int32_t *lmask;                   // moved this round and still active: the fits whose legs are recomputed
};

inline int64_t symv_packed_partials(int64_t P) {
  const int64_t T = (P + TBK - 1) / TBK;
  return T * T * TBK;
}
// y_b = A_b u_b and quad_b = u_b^T A_b u_b from the packed upper tiles of A_b (both triangles' contributions; only elements
// on or above the diagonal are read).  part: symv_packed_partials(P) doubles per fit.  No atomics: bitwise reproducible.
hipError_t launch_symv_packed(hipStream_t st, const double *apk, int64_t apk_stride, int64_t P, int32_t B, const double *u,
                              int64_t u_stride, double *part, double *y, int64_t y_stride, double *quad, int64_t q_stride,
                              const int32_t *active);
// dense [B][P][ld] -> packed tiles (the layout b_finalize_pack_kernel leaves behind); for lsqamdb_op_symv_packed
hipError_t launch_pack_dense(hipStream_t st, const double *A, int64_t ld, int64_t a_stride, int64_t P, int32_t B, double *apk,
                             int64_t apk_stride);
hipError_t launch_trs_init(hipStream_t st, int64_t P, int32_t B, const double *diag, const double *x, BTrs t);
hipError_t launch_trs_mask(hipStream_t st, int32_t B, BState s, BTrs t);
hipError_t launch_trs_grad(hipStream_t st, int64_t P, int32_t B, const double *gvec, int64_t g_stride, const double *diag, BTrs t,
                           const int32_t *mask);
hipError_t launch_trs_legs(hipStream_t st, int64_t P, int32_t B, int trs, const double *gvec, int64_t g_stride, const double *diag,
                           const double *v, int64_t v_stride, const int32_t *cholinfo, BTrs t, const int32_t *mask);
hipError_t launch_trs_step(hipStream_t st, int64_t P, int32_t B, int trs, const double *x, double *xt, double *dx, BTrs t,
                           const int32_t *active);
hipError_t launch_trs_decide(hipStream_t st, int32_t B, double factor_up, double factor_down, BState s, BTrs t);

}  // namespace lsqamd
