// Batched symmetric eigensolver for the covariance blocks the svdcut floor binds (2 <= B <= 256):
// the eigen-mode route of doc/source/overview.rst:1546-1606, which gvar takes for every block and
// which whiten.hip's Cholesky route has to hand back (status 1 / 2).  Those blocks are singular or
// nearly so (a covariance estimated from fewer samples than points), and they are the normal input
// of a correlated fit with an svdcut.
//
// Cyclic one-sided (Hestenes) Jacobi, ONE workgroup per block, grid = n_blocks:
//
//   G = A, V = I;  a rotation of the column pair (p, q) is chosen so that g_p . g_q becomes 0 and is
//   applied to the stacked columns [g; v].  G = A V throughout, so at convergence the columns of G are
//   orthogonal, |lambda_j| = |g_j| and sign(lambda_j) = sign(v_j . g_j); V is orthonormal by
//   construction, whatever the spectrum -- the null space of a singular block comes out as whatever
//   orthonormal basis the accumulated rotations give.
//
//   A sweep is B' - 1 steps (B' = B rounded up to even) of the round-robin tournament: every step holds
//   B' / 2 DISJOINT pairs, dealt to the workgroup's waves; the phantom index B of an odd B sits its
//   pair out.  One wave rotates one pair at a time: the lanes split the rows, the three dot products
//   are wave butterflies (every lane ends with the same bits, so the decision is wave-uniform), and
//   one barrier ends the step.
//
// Where the columns live (column j contiguous, so that the 64 lanes read consecutive words):
//   B <=  64   G and V in LDS                       (2 B (B + 1) doubles: 66.6 KB at 64)
//   B <= 128   G in LDS (132 KB at 128, of the CU's 160 KiB), V in a global slab that stays in L2
//   B <= 256   G and V in the global slab (1 MB per block at 256); a column changes hands between
//              waves only across the step's barrier, in front of which every wave drains its stores
// Larger blocks keep the host's LAPACK route (lsqfit_amd/whiten.py).
//
// What bounds it: the chain of (B' - 1) x sweeps barrier steps per block (255 x ~15 at B = 256), each
// a load - reduce - store round trip; the arithmetic is negligible (DESIGN.md 4.1's latency-bound
// family).  Blocks are independent, so a batch of 256 fills the chip.
//
// Singular input: columns of G shrink to rounding noise (~ eps |A|_F).  A pair is left alone when
// |g_p . g_q| <= tol |g_p| |g_q| OR either norm is at or below eps |A|_F: noise is not chased -- such a
// column IS a null vector to working precision (|A v| <= eps |A|_F), whatever it still overlaps with, and
// against a column 1e150 times its size the relative test would never be met.  The sweep
// loop is bounded (kMaxSweeps); a block that has not had a rotation-free sweep by then, whose
// eigenvalues are not finite, or one of whose columns is no eigenvector (see the lambda pass), ends
// with status 1 and the caller takes the host route for it.
#include <cmath>

#include "common.h"

namespace lsqamd {
namespace {

constexpr int kMaxSweeps = 30;
constexpr double kEps = 2.220446049250313e-16;

// all-lanes sums of three values (xor butterfly: IEEE addition commutes, so every lane holds the same bits)
__device__ __forceinline__ void wave_sum3(double &a, double &b, double &c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    c += __shfl_xor(c, o, 64);
  }
}

// RPL: rows per lane (B <= 64 RPL).  PLACE: 0 = G, V in LDS; 1 = G in LDS, V in the slab; 2 = both in the slab.
// A_b (symmetric, leading dimension lda) is read once and overwritten with V_b (eigenvectors as columns,
// ascending eigenvalue order).
template <int RPL, int PLACE>
__global__ __launch_bounds__(1024) void eigh_jacobi_kernel(double *A, int B, int64_t lda, int64_t strideA, double *slab,
                                                           int64_t strideS, double *lam_out, int32_t *sweeps_out,
                                                           int32_t *status_out) {
  extern __shared__ double lds[];
  __shared__ double lam_s[256];
  __shared__ int src_s[256];
  __shared__ double red_s[16];
  __shared__ int rot_cnt[2];
  __shared__ int mixed_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
  const int64_t blk = blockIdx.x;
  double *a = A + blk * strideA;
  const int64_t ldl = B + 1;     // LDS columns: odd stride, so the transposed read-out at the end is conflict-free too
  double *G, *V;
  int64_t ldg, ldv;
  if (PLACE == 0) {
    G = lds; V = lds + B * ldl; ldg = ldv = ldl;
  } else if (PLACE == 1) {
    G = lds; ldg = ldl; V = slab + blk * strideS; ldv = lda;
  } else {
    G = slab + blk * strideS; V = G + B * lda; ldg = ldv = lda;
  }
  // G = A (column j of a symmetric matrix is its row j), V = I, |A|_F^2
  double fro2 = 0.0;
  for (int idx = tid; idx < B * B; idx += nt) {
    const int j = idx / B, i = idx - j * B;
    const double v = a[j * lda + i];
    G[j * ldg + i] = v;
    V[j * ldv + i] = i == j ? 1.0 : 0.0;
    fro2 += v * v;
  }
  {
    double z0 = 0.0, z1 = 0.0;
    wave_sum3(fro2, z0, z1);
    if (lane == 0) red_s[wave] = fro2;
    if (tid == 0) rot_cnt[0] = rot_cnt[1] = mixed_s = 0;
  }
  __threadfence_block();
  __syncthreads();
  fro2 = 0.0;
  for (int w = 0; w < nw; ++w) fro2 += red_s[w];
  const double tol = (B > 4 ? B : 4) * kEps;
  const double floor2 = kEps * kEps * fro2;
  const int n = B + (B & 1);
  volatile int *cnt = rot_cnt;
  int prev[2] = {0, 0};
  int sweeps = 0;
  bool converged = false;
  for (int sweep = 0; sweep < kMaxSweeps && !converged; ++sweep) {
    for (int s = 0; s < n - 1; ++s) {
      for (int k = wave; k < n / 2; k += nw) {
        // round-robin: index n - 1 stays, the others walk round the table
        const int ia = k == 0 ? n - 1 : (s + k) % (n - 1);
        const int ib = k == 0 ? s : (s - k + (n - 1)) % (n - 1);
        const int p = ia < ib ? ia : ib, q = ia < ib ? ib : ia;
        if (q >= B) continue;                       // the phantom's partner rests
        double *gp = G + p * ldg, *gq = G + q * ldg;
        double xp[RPL], xq[RPL];
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const int i = lane + 64 * r;
          xp[r] = i < B ? gp[i] : 0.0;
          xq[r] = i < B ? gq[i] : 0.0;
          al += xp[r] * xp[r];
          be += xq[r] * xq[r];
          ga += xp[r] * xq[r];
        }
        wave_sum3(al, be, ga);
        // (written so that a NaN anywhere means "no rotation": the sweep loop then ends, and the block is reported unconverged)
        const bool rotate = fabs(ga) > tol * sqrt(al * be) && al > floor2 && be > floor2;
        if (!rotate) continue;
        const double zeta = (be - al) / (2.0 * ga);
        // (zeta^2 overflows for a column far below the other; 1 / (2 zeta) is the same number to rounding beyond 1e8)
        const double t = fabs(zeta) > 1.0e8 ? 0.5 / zeta : copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        double *vp = V + p * ldv, *vq = V + q * ldv;
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const int i = lane + 64 * r;
          if (i < B) {
            const double yp = vp[i], yq = vq[i];
            gp[i] = c * xp[r] - sn * xq[r];
            gq[i] = sn * xp[r] + c * xq[r];
            vp[i] = c * yp - sn * yq;
            vq[i] = sn * yp + c * yq;
          }
        }
        if (lane == 0) atomicAdd(&rot_cnt[sweep & 1], 1);
      }
      __threadfence_block();      // columns change hands at the barrier: this wave's stores are drained in front of it
      __syncthreads();
    }
    // rotations of this sweep: counter (sweep & 1) is next written two sweeps on, behind barriers every wave has to pass
    // after this read, so all threads see one value and leave the loop together
    const int now = cnt[sweep & 1];
    sweeps = sweep + 1;
    converged = now == prev[sweep & 1];
    prev[sweep & 1] = now;
  }
  // lambda_j = sign(v_j . g_j) |g_j|
  for (int j = wave; j < B; j += nw) {
    double nrm2 = 0.0, dot = 0.0, z = 0.0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      const int i = lane + 64 * r;
      const double g = i < B ? G[j * ldg + i] : 0.0, v = i < B ? V[j * ldv + i] : 0.0;
      nrm2 += g * g;
      dot += g * v;
    }
    wave_sum3(nrm2, dot, z);
    if (lane == 0) {
      const double nrm = sqrt(nrm2);
      lam_s[j] = dot < 0.0 ? -nrm : nrm;
      // Orthogonal columns of G = A V diagonalise A^2: eigenvalues +l and ~ -l of an indefinite block are degenerate
      // there, and a mixture of their eigenvectors passes the rotation test.  For an eigenvector v . g = lambda, so
      // |v . g| = |g| up to the rounding of the dot products; a column that fails this is not one.
      if (fabs(nrm - fabs(dot)) > 1.5e-8 * nrm + 64.0 * B * kEps * sqrt(fro2)) mixed_s = 1;
    }
  }
  for (int j = tid; j < B; j += nt) src_s[j] = 0;   // (NaN eigenvalues can share a rank: no slot is left unset)
  __syncthreads();
  // ascending order by rank (ties by index): src_s[rank] = column
  for (int j = tid; j < B; j += nt) {
    const double lj = lam_s[j];
    int rank = 0;
    for (int k = 0; k < B; ++k) {
      const double lk = lam_s[k];
      rank += (lk < lj || (lk == lj && k < j)) ? 1 : 0;
    }
    src_s[rank] = j;
  }
  __syncthreads();
  for (int idx = tid; idx < B * B; idx += nt) {
    const int i = idx / B, r = idx - i * B;
    a[i * lda + r] = V[src_s[r] * ldv + i];
  }
  for (int r = tid; r < B; r += nt) lam_out[blk * B + r] = lam_s[src_s[r]];
  if (tid == 0) {
    bool finite = true;
    for (int j = 0; j < B; ++j) finite = finite && fabs(lam_s[j]) < 1.0e300;
    sweeps_out[blk] = sweeps;
    status_out[blk] = converged && finite && !mixed_s ? 0 : 1;
  }
}

template <int RPL, int PLACE>
hipError_t launch_one(hipStream_t st, double *A, int64_t B, int64_t lda, int64_t strideA, int32_t nb, double *slab,
                      double *lam, int32_t *sweeps, int32_t *status) {
  const size_t lds = sizeof(double) * (size_t)((PLACE == 0 ? 2 : PLACE == 1 ? 1 : 0) * B * (B + 1));
  if (lds) {
    static PerDeviceMax lds_set;   // per device, thread-safe (common.h)
    const void *kfn = reinterpret_cast<const void *>(eigh_jacobi_kernel<RPL, PLACE>);
    const hipError_t e = lds_set.ensure(lds, [kfn](size_t want) {
      return hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
    });
    if (e != hipSuccess) return e;
  }
  // waves: the step's (B + 1) / 2 pairs in as few rounds as 16 waves allow, the rounds evenly filled
  const int pairs = (int)((B + 1) / 2), rounds = (pairs + 15) / 16, waves = (pairs + rounds - 1) / rounds;
  hipLaunchKernelGGL((eigh_jacobi_kernel<RPL, PLACE>), dim3((unsigned)nb), dim3((unsigned)(64 * waves)), lds, st, A, (int)B,
                     lda, strideA, slab, (int64_t)eigh_blocks_slab_doubles(B, lda), lam, sweeps, status);
  return hipGetLastError();
}

}  // namespace

size_t eigh_blocks_slab_doubles(int64_t B, int64_t lda) {
  return B <= 64 ? 0 : (size_t)((B <= 128 ? 1 : 2) * B * lda);
}

hipError_t launch_eigh_blocks(hipStream_t st, double *A, int64_t B, int64_t lda, int64_t strideA, int32_t nb, double *slab,
                              double *lam, int32_t *sweeps, int32_t *status) {
  if (B < 2 || B > kEighBlocksMax || nb < 1 || lda < B || (B > 64 && !slab)) return hipErrorInvalidValue;
  if (B <= 64) return launch_one<1, 0>(st, A, B, lda, strideA, nb, slab, lam, sweeps, status);
  if (B <= 128) return launch_one<2, 1>(st, A, B, lda, strideA, nb, slab, lam, sweeps, status);
  return launch_one<4, 2>(st, A, B, lda, strideA, nb, slab, lam, sweeps, status);
}

}  // namespace lsqamd
