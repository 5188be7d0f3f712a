// fp64 MFMA GEMM in "TN" form for gfx950 (MI355X):
//
//     C[M x N] = alpha * sum_k X[k][m] * Y[k][n] + beta * C        (row-major)
//
// This one kernel carries every dense contraction of the LM step:
//   J^T J            X = Y = J                       (replaces gsl_blas_dsyrk in GSL's
//                                                     cholesky solver init, reached from
//                                                     src/lsqfit/_gsl.pyx:677)
//   whitening        X = W_b^T, Y = raw Jacobian     (replaces `dot`, _utilities.pyx:20-36,90-93)
//   Cholesky panel   X = inv(U_kk), Y = row panel
//   trailing update  X = Y = row panel, alpha = -1, beta = 1
//   covariance       X = Y = U^-T                     (replaces gsl_multifit_nlinear_covar,
//                                                     _gsl.pyx:704-706)
//
// Design (MI355X_MICROARCH / cdna_hip_programming guides):
//   * v_mfma_f64_16x16x4_f64: A operand lane l = A[l&15][l>>4], B operand lane l =
//     B[l>>4][l&15], C/D lane l reg r = C[(l>>4) + 4r][l&15].  With k-major
//     operands both fragments are plain row reads of the staged tile -- no
//     transpose anywhere, and global loads are full 1 KiB rows (coalesced).
//   * 128x128 block tile, BK = 16, 256 threads = 4 waves in 2x2, each wave a
//     64x64 sub-tile = 4x4 MFMA tiles (128 accumulator VGPRs): 16 MFMAs (1024
//     matrix-pipe cycles) per 8 ds_read_b64.
//   * LDS rows padded 128 -> 144 doubles so the four k-rows a wave reads in one
//     ds_read_b64 fall in different bank halves (stride 288 dwords = 32 mod 64).
//   * two LDS stages (73.7 KB) -> 2 blocks / CU; global loads for stage t+1 are
//     issued before the MFMAs of stage t and written to LDS after them.
//   * split-K over rows (the long dimension, N_data) into per-split slabs summed
//     by a second pass: deterministic, and gives >> 256 workgroups.
#include <cstdlib>

#include "common.h"
#include <type_traits>
#include <vector>
#include "devmath.h"

namespace lsqamd {

#ifdef LSQAMD_SYRK_STAMPS
// developer build (tools/build_variant.sh syrkstamps gemm_tn_f64.hip -DLSQAMD_SYRK_STAMPS; tools/syrk_schedule.py): every
// workgroup of the work-list launch leaves (start, end) in 100 MHz ticks, XCC_ID, HW_ID and its list index
__device__ unsigned long long *g_syrk_stamps = nullptr;
#endif

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int BM = 128, BN = 128, BK = 16;
constexpr int LDT = BM + 16;                       // padded LDS row (doubles)
constexpr int STAGE = 2 * BK * LDT;                // X tile + Y tile per stage (doubles)
constexpr size_t GEMM_LDS_BYTES = 2 * STAGE * sizeof(double);

struct GemmDev {
  const double *X, *Y;
  double *C;
  int64_t M, N, K, ldx, ldy, ldc;
  double alpha, beta;
  int64_t sx, sy, sc;
  int32_t tiles_n, upper_only, x_upper_tri, xy_lower_tri, splits;
  int32_t tiles_m, pair_rows;
  int32_t tri_halves;    // XTRI interior launch with two K-halves per tile row (grid.y = 2), see GemmTN::tri_halves
  int32_t xcd_groups;    // XTRI interior launch as a 1-D grid: the tile columns of one (tile row [pair], K-half) on ONE XCD; = number of tile rows [pairs]
  int32_t syrk_diag;     // WORKMAP launch with X == Y: diagonal tiles take the triangular schedule (see kernel)
  int32_t vec_x, vec_y;  // operand rows are 16-byte aligned -> dwordx4 loads
  int64_t kchunk, split_stride;
  const int32_t *work_map;  // optional: work item -> (tm, tn, split, -) with XCD-aware order
  int32_t n_work;
  const int32_t *batch_active;  // optional: skip batch entries whose flag is 0
  double *colsum_out;           // optional (XTRI interior kernel): fused column sums, see GemmTN
  int64_t colsum_ld, colsum_rcol;
  int32_t *done_ctr;            // optional (WORKMAP + SIGNAL): done_ctr[group - 1] += 1 when an entry whose 4th word is `group` is complete
};

// Branch-free staging loads.  Out-of-range rows/columns are CLAMPED to a valid
// address and zeroed when the registers are written to LDS, i.e. after the wait
// the compiler places in front of the ds_write -- so the global loads of stage
// t+1 stay in flight across the MFMAs of stage t (a mask applied at load time
// forces an s_waitcnt vmcnt(0) right behind every load).
template <bool VEC>
__device__ __forceinline__ v2d load2(const double *rowptr, int64_t i0, int64_t i1) {
  if (VEC) return *reinterpret_cast<const v2d *>(rowptr + i0);  // i0 even, i0 + 1 < ld
  v2d v;
  v.x = rowptr[i0];
  v.y = rowptr[i1];
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void gemm_tn_f64_kernel(GemmDev g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn, split;
  if (g.work_map) {
    // Workgroup b runs on XCD b % 8 (observed dispatch order; speed only, never correctness).
    // Give every XCD one contiguous run of the work list, whose neighbours share operand
    // panels, so that the 64 workgroups resident on an XCD hit its private L2.
    const int nw = g.n_work, bid = blockIdx.x;
    const int xcd = bid & 7, q = nw >> 3, r = nw & 7;
    const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int4 e = reinterpret_cast<const int4 *>(g.work_map)[w];
    tm = e.x; tn = e.y; split = e.z;
  } else {
    tm = blockIdx.x / g.tiles_n;
    tn = blockIdx.x % g.tiles_n;
    split = blockIdx.y;
  }
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  if (g.upper_only && n0 + BN <= m0) return;  // tile strictly below the diagonal

  const int64_t b = blockIdx.z;
  if (g.batch_active && !g.batch_active[b]) return;
  const double *X = g.X + b * g.sx;
  const double *Y = g.Y + b * g.sy;
  double *C = g.C + b * g.sc + (int64_t)split * g.split_stride;

  int64_t kb = (int64_t)split * g.kchunk;
  int64_t ke = kb + g.kchunk < g.K ? kb + g.kchunk : g.K;
  if (g.x_upper_tri) {  // X[k][m] = 0 for k > m
    const int64_t lim = m0 + BM;
    if (ke > lim) ke = lim;
  }
  if (g.xy_lower_tri) {  // X[k][m] = 0 for m > k, same for Y
    int64_t lo = m0 > n0 ? m0 : n0;
    lo -= lo % BK;
    if (kb < lo) kb = lo;
  }

  v4d acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

  // staging map: thread -> (row group, 2 columns); column validity is loop-invariant
  const int c2 = (tid & 63) * 2;
  const int rg = tid >> 6;
  const int64_t xc = m0 + c2, yc = n0 + c2;
  const bool x0ok = xc < g.M, x1ok = xc + 1 < g.M;
  const bool y0ok = yc < g.N, y1ok = yc + 1 < g.N;
  // always-readable indices: VEC -> aligned pair inside the (even) leading dimension,
  // scalar -> each element clamped to the last valid column
  const int64_t xi0 = VEC ? (xc < g.ldx - 2 ? xc : g.ldx - 2) : (xc < g.M ? xc : g.M - 1);
  const int64_t xi1 = xc + 1 < g.M ? xc + 1 : g.M - 1;
  const int64_t yi0 = VEC ? (yc < g.ldy - 2 ? yc : g.ldy - 2) : (yc < g.N ? yc : g.N - 1);
  const int64_t yi1 = yc + 1 < g.N ? yc + 1 : g.N - 1;
  v2d xr[4], yr[4];

  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t row = k0 + rg + 4 * i;
      row = row < ke ? row : ke - 1;
      xr[i] = load2<VEC>(X + row * g.ldx, xi0, xi1);
      yr[i] = load2<VEC>(Y + row * g.ldy, yi0, yi1);
    }
  };
  auto sstore = [&](int buf, int64_t k0) {
    double *Xs = smem + buf * STAGE;
    double *Ys = Xs + BK * LDT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rg + 4 * i;
      const bool rok = k0 + row < ke;
      v2d xv, yv;
      xv.x = (rok && x0ok) ? xr[i].x : 0.0;
      xv.y = (rok && x1ok) ? xr[i].y : 0.0;
      yv.x = (rok && y0ok) ? yr[i].x : 0.0;
      yv.y = (rok && y1ok) ? yr[i].y : 0.0;
      *reinterpret_cast<v2d *>(Xs + row * LDT + c2) = xv;
      *reinterpret_cast<v2d *>(Ys + row * LDT + c2) = yv;
    }
  };

  const int fr = lane & 15, fq = lane >> 4;
  if (kb < ke) {
    gload(kb);
    sstore(0, kb);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t k0 = kb; k0 < ke; k0 += BK) {
    const bool more = k0 + BK < ke;
    if (more) gload(k0 + BK);
    const double *Xs = smem + cur * STAGE;
    const double *Ys = Xs + BK * LDT;
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const int kr = kk * 4 + fq;
      double a[4], bb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Xs[kr * LDT + wm * 64 + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < 4; ++j) bb[j] = Ys[kr * LDT + wn * 64 + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
    if (more) sstore(cur ^ 1, k0 + BK);
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: lane holds rows fq + 4r, column fr of each 16x16 sub-tile.  With beta != 0
  // the 16 C values of a sub-tile row are loaded together (one branch, loads in flight
  // at once) -- a per-element "if (beta) load" costs one memory round trip per element.
  const double alpha = g.alpha;
  const double beta = g.splits > 1 ? 0.0 : g.beta;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double cv[4][4];
    if (beta != 0.0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t col = n0 + wn * 64 + j * 16 + fr;
          const int64_t row = m0 + wm * 64 + i * 16 + fq + 4 * r;
          const bool ok = col < g.N && row < g.M;
          cv[j][r] = C[(ok ? row : 0) * g.ldc + (ok ? col : 0)];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t col = n0 + wn * 64 + j * 16 + fr;
      if (col >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + wm * 64 + i * 16 + fq + 4 * r;
        if (row >= g.M) continue;
        double v = alpha * acc[i][j][r];
        if (beta != 0.0) v += beta * cv[j][r];
        C[row * g.ldc + col] = v;
      }
    }
  }
}

// Interior fast path: every tile full (M, N multiples of 128), every K-range a multiple of
// BK, 16-byte aligned rows.  Operand rows go HBM -> LDS directly (global_load_lds_dwordx4:
// one wave instruction lands one 1 KiB tile row, lane l -> bytes [16 l, 16 l + 16) of the
// row, so the padded row stride costs nothing), no staging VGPRs, no ds_write pass, no
// masks; row pointers advance by a constant instead of being recomputed.
// XTRI (X upper triangular, the whitening product with X = W_b^T): the 16-row MFMA strips of
// the two wave rows are interleaved (strip 2i + wm instead of 4 wm + i) and a strip skips the
// k-steps that lie entirely below its rows -- X is zero there.  Interleaving matters: with
// contiguous 64-row halves the lower half would still do 81 % of the k-steps of a diagonal tile
// while the upper half idles; interleaved, the busier wave row does 62 %.
// WORKMAP: the split-K J^T J launch (XCD-aware work list).  A separate instantiation so that it
// shows up under its own name in kernel traces (the Cholesky's trailing updates use <false, false>).
// Diagonal tiles of that launch (X == Y, tm == tn) are symmetric: the lower-left 64 x 64 quadrant is
// the transpose of the upper-right one and the 16 x 16 sub-tiles below the diagonal of the two
// diagonal quadrants repeat the ones above.  Schedule: waves 0 and 3 compute the 10 sub-tiles
// i <= j of their quadrants, waves 1 and 2 each take two 16-row strips of the upper-right quadrant
// (8 sub-tiles), i.e. at most 10 MFMAs per k-step and wave instead of 16, the Y tile is not staged
// (it is the X tile), and the epilogue writes every value to (row, col) and (col, row): the tile in
// the slab is bit-identical to the one the full schedule writes (same products, same k order).
// CS (with WORKMAP, diagonal tiles on the triangular schedule): the workgroup of diagonal tile (tm, tm, split)
// also forms sum_k X[k][m] * X[k][rcol] over its K-range for its 128 columns m -- J^T f out of the tile rows
// that are in LDS anyway, so the gradient costs no second pass over J.  The residual column's 16 values of a
// stage land in the (unused) Y half of the stage buffer; column rcol itself gets sum_k X[k][rcol]^2 from tile 0.
// colsum_out[(b * splits + split) * colsum_ld + m]: per-split partials, summed in split order by the caller.
// SIGNAL (with WORKMAP): the work list's 4th word names the entry's exchange group (1-based); when the entry's tile is in its
// slab the workgroup adds one to done_ctr[group - 1] with release semantics -- a one-wave kernel on another stream of the
// handle waits for the count of a group's entries (eval.hip: the grouped exchange without splitting this launch).
template <bool XTRI, bool WORKMAP, bool CS = false, bool SIGNAL = false>
__global__ __launch_bounds__(256, 2) void gemm_tn_f64_interior_kernel(GemmDev g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  // Uniform control: the wave index and the work-list entry are the same in every lane, but the compiler cannot see that
  // (tid >> 6; a per-lane load), so they are made uniform by hand.  Everything derived from them -- m0, n0, kb, ke, the
  // diagonal role, the C base, the operand row bases, the LDS destinations of the staging loads -- then lives in scalar
  // registers and the k loop's control is scalar compares on a 32-bit stage count.
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn, split;
  int sig_group = 0;
#ifdef LSQAMD_SYRK_STAMPS
  const unsigned long long stamp0 = __builtin_amdgcn_s_memrealtime();
  int stamp_w = -1;
#endif
  if (WORKMAP) {
    // (as in gemm_tn_f64_kernel: workgroup b runs on XCD b % 8; every XCD walks one contiguous run of the list)
    const int nw = g.n_work, bid = blockIdx.x;
    const int xcd = bid & 7, q = nw >> 3, r = nw & 7;
    const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
#ifdef LSQAMD_SYRK_STAMPS
    stamp_w = w;
#endif
    const int4 e = reinterpret_cast<const int4 *>(g.work_map)[w];
    tm = __builtin_amdgcn_readfirstlane(e.x);
    tn = __builtin_amdgcn_readfirstlane(e.y);
    split = __builtin_amdgcn_readfirstlane(e.z);
    if (SIGNAL) sig_group = __builtin_amdgcn_readfirstlane(e.w);
  } else if (XTRI && g.xcd_groups) {
    // Workgroup b runs on XCD b % 8.  With the tile column as the fastest index (and 8 of them) every XCD would own ONE
    // tile column and read ALL of X for it -- config 3's triangular whitening matrix went past the L2 eight times (L2 hit
    // 12 %, 3.9 GB per launch, r05_c3_pmc.json).  Here the tile columns of one (tile row [pair], K-half) are neighbours on
    // ONE XCD: they walk the same rows of X at the same pace and share them in its L2.
    const int L = blockIdx.x, xcd = L & 7, sl = L >> 3;
    const int gidx = xcd + 8 * (sl / g.tiles_n);
    tn = sl % g.tiles_n;
    tm = gidx % g.xcd_groups;
    split = gidx / g.xcd_groups;
  } else {
    tm = blockIdx.x / g.tiles_n;
    tn = blockIdx.x % g.tiles_n;
    split = blockIdx.y;
  }
  // pair_rows (triangular X with many tile rows): this workgroup does tile rows tm and
  // T-1-tm one after the other, so every workgroup sees the same total K (the k-range of a
  // tile row grows with tm: unpaired, the last rows take 64x as long as the first)
  const int tm_other = (XTRI && g.pair_rows) ? g.tiles_m - 1 - tm : tm;
  const int npass = tm_other != tm ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
  if (pass >= 1) {
    tm = tm_other;
    __syncthreads();
  }
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  if (g.upper_only && n0 + BN <= m0) return;
  const int64_t b = blockIdx.z;
  if (g.batch_active && !g.batch_active[b]) return;
  double *C = g.C + b * g.sc + (int64_t)split * g.split_stride;
  int64_t kb = (int64_t)split * g.kchunk;
  int64_t ke = kb + g.kchunk < g.K ? kb + g.kchunk : g.K;
  if (g.x_upper_tri) {
    const int64_t lim = m0 + BM;
    if (ke > lim) ke = lim;
  }
  if (g.xy_lower_tri) {
    int64_t lo = m0 > n0 ? m0 : n0;
    lo -= lo % BK;
    if (kb < lo) kb = lo;
  }
  if (XTRI && g.tri_halves) {   // the tile row's own K-range [0, m0 + 128) cut in two: split 0 the lower half, split 1 the upper
    const int64_t lim = m0 + BM, h = (lim >> 1) & ~(int64_t)(BK - 1);
    kb = split ? h : 0;
    ke = split ? lim : h;
  }

  v4d acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

  const bool diag = WORKMAP && !XTRI && g.syrk_diag && tm == tn;
  // tile rows / columns of this wave's 16-wide strips: strip i -> rows arow0 + 16 i, strip j -> columns bcol0 + 16 j
  const int arow0 = diag ? (wave == 2 ? 32 : (wave == 3 ? 64 : 0)) : wm * 64;
  const int bcol0 = diag ? (wave == 0 ? 0 : 64) : wn * 64;

  // wave w stages rows w, w+4, w+8, w+12 of both tiles; lane -> 2 columns
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  // (xb, yb: uniform row bases, advanced per stage on the scalar unit; lane_off: this lane's 16 bytes of a row)
  const char *xb = reinterpret_cast<const char *>(g.X + b * g.sx + (kb + wave) * g.ldx + m0);
  const char *yb = reinterpret_cast<const char *>(g.Y + b * g.sy + (kb + wave) * g.ldy + n0);
  const int64_t xstep = 4 * g.ldx * (int64_t)sizeof(double), ystep = 4 * g.ldy * (int64_t)sizeof(double);
  uint32_t lane_off = 16u * (uint32_t)lane;
  const int nst = kb < ke ? (int)((ke - kb + BK - 1) >> 4) : 0;   // K stages of this entry (BK = 16)
  // CS: lanes 0..31 of wave 1 fetch the 16 residuals of a stage as 32 dwords (lane -> row lane / 2, half lane & 1)
  const char *fp = reinterpret_cast<const char *>(g.X + b * g.sx + (kb + (lane >> 1)) * g.ldx + g.colsum_rcol) + 4 * (lane & 1);
  const int64_t fstep = (int64_t)BK * g.ldx * (int64_t)sizeof(double);
  double cs = 0.0, cs2 = 0.0;

  // Staging addresses: uniform row base + loop-invariant 32-bit lane offset.  The builtin is enough: with the address in
  // this form the compiler picks the scalar-base encoding (global_load_lds_dwordx4 v_off, s[base:base+1]) and, the
  // buffer index being a compile-time value and `wave` uniform, each LDS destination is a scalar moved to m0.  The
  // encoding is chosen per basic block and only when the 32 -> 64-bit extension of the lane offset is in the block of
  // the load: the empty statement (no instruction) redefines lane_off here so that the extension is not hoisted.
  auto stage = [&](auto buf_tag) {
    constexpr int buf = decltype(buf_tag)::value;
    asm volatile("" : "+v"(lane_off));
    double *Xs = smem + buf * STAGE + wave * LDT;
    double *Ys = Xs + BK * LDT;
    if (diag) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds((glb_void *)(xb + i * xstep + lane_off), (lds_void *)(Xs + 4 * i * LDT), 16, 0, 0);
      if (CS && wave == 1) {
        if (lane < 32)
          __builtin_amdgcn_global_load_lds((glb_void *)fp, (lds_void *)(smem + buf * STAGE + BK * LDT), 4, 0, 0);
        fp += fstep;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_global_load_lds((glb_void *)(xb + i * xstep + lane_off), (lds_void *)(Xs + 4 * i * LDT), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void *)(yb + i * ystep + lane_off), (lds_void *)(Ys + 4 * i * LDT), 16, 0, 0);
      }
    }
    xb += 4 * xstep;
    yb += 4 * ystep;
  };

  // weights of the fused column sums: fetched now, used in the epilogue (latency hidden by the k loop)
  const bool fuse = XTRI && g.colsum_out != nullptr;
  double wreg = 0.0;
  if (fuse && tid < BM) wreg = (g.C + b * g.sc)[(m0 + tid) * g.ldc + g.colsum_rcol];
  const int fr = lane & 15, fq = lane >> 4;
  if (nst > 0) stage(std::integral_constant<int, 0>{});
  __syncthreads();
  // ROLE 0: all 16 sub-tiles; 1: sub-tiles i <= j (diagonal quadrant of a diagonal tile); 2: strips i < 2
  auto kloop = [&](auto role_tag) {
    constexpr int ROLE = decltype(role_tag)::value;
    // fragment bases per (buffer, k-step): a k-step is 4608 bytes, beyond the reach of a ds_read2_b64 offset, so each gets
    // its own address register, set once (the empty statements keep the compiler from recomputing them in every stage)
    typedef const __attribute__((address_space(3))) double lds_cdouble;
    lds_cdouble *ap[2][BK / 4], *bp[2][BK / 4];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        const double *Xk = smem + c * STAGE + (kk * 4 + fq) * LDT + fr;
        ap[c][kk] = (lds_cdouble *)(Xk + (XTRI ? wm * 16 : arow0));
        bp[c][kk] = (lds_cdouble *)(Xk + (ROLE == 0 ? BK * LDT : 0) + bcol0);
        asm volatile("" : "+v"(ap[c][kk]), "+v"(bp[c][kk]));
      }
    // one K stage out of buffer `cur` (a compile-time value: the LDS reads are base register + immediate)
    // TRI (XTRI only): 0 = a full stage, every strip takes every k-step; 1 = stage ts = 0..7 of the tile row's own 128
    // k-values, k0 = m0 + 16 ts.  X[k][m] = 0 for k > m: strip t = 2 i + wm (rows m0 + 16 t .. + 15) sees nothing from
    // k-steps k0 + 4 kk > m0 + 16 t + 15, i.e. it takes all four k-steps of the stage when t >= ts and none otherwise.
    // One 32-bit test of uniform values per strip (a scalar compare and branch) with the strip as the outer loop: every
    // accumulator still receives its k-steps in ascending order, so the sums are the same.
    auto body = [&](auto cur_tag, auto tri_tag, const int ts, const bool more) {
      constexpr int cur = decltype(cur_tag)::value;
      constexpr bool TRI = XTRI && decltype(tri_tag)::value != 0;
      if (more) stage(std::integral_constant<int, cur ^ 1>{});
      const double *Xs = smem + cur * STAGE;
      if (TRI) {
        double bb[BK / 4][4];
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk)
#pragma unroll
          for (int j = 0; j < 4; ++j) bb[kk][j] = bp[cur][kk][j * 16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (2 * i + wm < ts) continue;
          double a[BK / 4];
#pragma unroll
          for (int kk = 0; kk < BK / 4; ++kk) a[kk] = ap[cur][kk][2 * i * 16];
#pragma unroll
          for (int kk = 0; kk < BK / 4; ++kk)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bb[kk][j], acc[i][j], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
          double a[4], bb[4];
#pragma unroll
          for (int i = 0; i < (ROLE == 2 ? 2 : 4); ++i) a[i] = ap[cur][kk][(XTRI ? 2 * i : i) * 16];
#pragma unroll
          for (int j = 0; j < 4; ++j) bb[j] = bp[cur][kk][j * 16];
#pragma unroll
          for (int i = 0; i < (ROLE == 2 ? 2 : 4); ++i)
#pragma unroll
            for (int j = (ROLE == 1 ? i : 0); j < 4; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
        }
      }
      if (CS && ROLE != 0) {   // thread -> column tid & 127, rows 8 (tid >> 7) .. + 7 of the stage
        const double *Fs = Xs + BK * LDT + 8 * (tid >> 7);
        const double *Xc = Xs + 8 * (tid >> 7) * LDT + (tid & 127);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const double fv = Fs[r];
          cs = fma(Xc[r * LDT], fv, cs);
          cs2 = fma(fv, fv, cs2);
        }
      }
      __syncthreads();
    };
    // the full stages (all of them unless XTRI; XTRI: those below the tile row's own k-values, k0 + BK <= m0): the loop
    // unrolled by two (buffers 0, 1), then the peeled last stage of an odd count (a one-stage entry is that stage alone)
    using c0_tag = std::integral_constant<int, 0>;
    using c1_tag = std::integral_constant<int, 1>;
    int nfull = nst;
    if (XTRI) {
      const int64_t below = kb < m0 ? (m0 - kb) >> 4 : 0;
      nfull = below < nst ? (int)below : nst;
    }
    int s = 0;
    for (; s + 1 < nfull; s += 2) {
      body(c0_tag{}, c0_tag{}, 0, true);
      body(c1_tag{}, c0_tag{}, 0, s + 2 < nst);
    }
    if (s < nfull) body(c0_tag{}, c0_tag{}, 0, s + 1 < nst);
    if (XTRI && nfull < nst) {
      // the (up to eight) triangular stages t0 .. t1 - 1 (stages past the eighth would multiply zeros only), again
      // unrolled by two: first one stage out of buffer 1 if that is where the full stages ended
      const int t1 = (int)((kb + (int64_t)nst * BK - m0) >> 4);
      int t = t1 - (nst - nfull);
      if (nfull & 1) {
        body(c1_tag{}, c1_tag{}, t, t + 1 < t1);
        ++t;
      }
      for (; t + 1 < t1; t += 2) {
        body(c0_tag{}, c1_tag{}, t, true);
        body(c1_tag{}, c1_tag{}, t + 1, t + 2 < t1);
      }
      if (t < t1) body(c0_tag{}, c1_tag{}, t, false);
    }
  };
  if (WORKMAP && !XTRI && diag) {
    if (wave == 0 || wave == 3) kloop(std::integral_constant<int, 1>{});
    else kloop(std::integral_constant<int, 2>{});
    // epilogue of a diagonal tile: each value to (row, col) and to its mirror image
    const double alpha = g.alpha;
    const bool tri = wave == 0 || wave == 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!tri && i >= 2) break;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (tri && j < i) continue;
        const int64_t col = n0 + bcol0 + j * 16 + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = m0 + arow0 + i * 16 + fq + 4 * r;
          const double v = alpha * acc[i][j][r];
          C[row * g.ldc + col] = v;
          if (!(tri && i == j)) C[col * g.ldc + row] = v;
        }
      }
    }
    if (CS) {   // (the k loop ended on a barrier: the stage buffers are free)
      smem[tid] = cs;
      if ((tid & 127) == 0) smem[256 + (tid >> 7)] = cs2;
      __syncthreads();
      double *out = g.colsum_out + (b * g.splits + split) * g.colsum_ld;
      if (tid < BM) out[m0 + tid] = smem[tid] + smem[tid + 128];
      if (tm == 0 && tid == 0) out[g.colsum_rcol] = smem[256] + smem[257];
    }
    continue;
  }
  kloop(std::integral_constant<int, 0>{});

  const double alpha = g.alpha;
  const double beta = g.splits > 1 ? 0.0 : g.beta;
  double *wcol = smem;             // [128] weights of this tile's rows (LDS is free after the k loop)
  double *red = smem + 128;        // [4 waves][64] partial column sums
  if (fuse) {
    if (tid < BM) wcol[tid] = wreg;
    __syncthreads();
  }
  double sj[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rloc = (XTRI ? (2 * i + wm) * 16 : wm * 64 + i * 16) + fq;
    const int64_t rbase = m0 + rloc;
    double cv[4][4];
    if (beta != 0.0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          cv[j][r] = C[(rbase + 4 * r) * g.ldc + n0 + wn * 64 + j * 16 + fr];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double w = fuse ? wcol[rloc + 4 * r] : 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double v = alpha * acc[i][j][r];
        if (beta != 0.0) v += beta * cv[j][r];
        C[(rbase + 4 * r) * g.ldc + n0 + wn * 64 + j * 16 + fr] = v;
        if (XTRI) sj[j] += v * w;
      }
    }
  }
  if (fuse) {
    // fused J^T f: the tile times the weight column of its rows, summed over the rows -- in-thread
    // over (i, r) above, across the four 16-lane groups by two butterfly steps, across the two
    // wave rows through LDS
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sj[j] += __shfl_xor(sj[j], 16, 64);
      sj[j] += __shfl_xor(sj[j], 32, 64);
    }
    if (fq == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave * 64 + j * 16 + fr] = sj[j];
    }
    __syncthreads();
    if (wm == 0 && fq == 0) {
      double *out = g.colsum_out + (b * g.tiles_m + tm) * g.colsum_ld + n0 + wn * 64;
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j * 16 + fr] = red[wave * 64 + j * 16 + fr] + red[(wave + 2) * 64 + j * 16 + fr];
    }
  }
  }  // pass
  if (SIGNAL && WORKMAP && sig_group > 0 && g.done_ctr) {
    // the guide's counter hand-off (cdna_hip_programming.md 6 G16 / 5.x "in-launch split-K reduction"): every wave drains its
    // own stores, barrier, ONE lane issues the agent-scope release (buffer_wbl2: this XCD's L2 is not coherent with the one
    // the consumer kernel will read through), waits for it, then counts with a RELAXED add.  NOT __threadfence() in every
    // thread: that is a write-back AND an invalidate per thread -- it cost the product 6 % (the panels' L2 lines went with it)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_fetch_add(g.done_ctr + (sig_group - 1), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#ifdef LSQAMD_SYRK_STAMPS
  if (WORKMAP && g_syrk_stamps && tid == 0) {
    __builtin_amdgcn_s_waitcnt(0);
    unsigned long long *o = g_syrk_stamps + 5 * (size_t)blockIdx.x;
    o[0] = stamp0;
    o[1] = __builtin_amdgcn_s_memrealtime();
    o[2] = __builtin_amdgcn_s_getreg((3 << 11) | 20);
    o[3] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    o[4] = (unsigned long long)stamp_w;
  }
#endif
}

// 64 x 64-tile variant for the latency-bound contractions of the Cholesky family (K = 128,
// a handful of 128-tiles): four times the workgroups, a quarter of the MFMA chain each.
// Same contract as gemm_tn_f64_kernel (edges, triangular flags, beta, batch).
constexpr int TS = 64;
constexpr int LDS_S = TS + 16;
constexpr int STAGE_S = 2 * BK * LDS_S;
constexpr size_t GEMM_LDS_BYTES_S = 2 * STAGE_S * sizeof(double);

template <bool VEC>
__global__ __launch_bounds__(256, 4) void gemm_tn_f64_small_kernel(GemmDev g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x / g.tiles_n, tn = blockIdx.x % g.tiles_n;
  const int split = blockIdx.y;
  const int64_t m0 = (int64_t)tm * TS, n0 = (int64_t)tn * TS;
  if (g.upper_only && n0 + TS <= m0) return;
  const int64_t b = blockIdx.z;
  if (g.batch_active && !g.batch_active[b]) return;
  const double *X = g.X + b * g.sx;
  const double *Y = g.Y + b * g.sy;
  double *C = g.C + b * g.sc + (int64_t)split * g.split_stride;
  int64_t kb = (int64_t)split * g.kchunk;
  int64_t ke = kb + g.kchunk < g.K ? kb + g.kchunk : g.K;
  if (g.x_upper_tri) {
    const int64_t lim = m0 + TS;
    if (ke > lim) ke = lim;
  }
  if (g.xy_lower_tri) {
    int64_t lo = m0 > n0 ? m0 : n0;
    lo -= lo % BK;
    if (kb < lo) kb = lo;
  }
  v4d acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

  const int c2 = (tid & 31) * 2;
  const int rg = tid >> 5;  // 0..7 ; rows rg, rg + 8
  const int64_t xc = m0 + c2, yc = n0 + c2;
  const bool x0ok = xc < g.M, x1ok = xc + 1 < g.M;
  const bool y0ok = yc < g.N, y1ok = yc + 1 < g.N;
  const int64_t xi0 = VEC ? (xc < g.ldx - 2 ? xc : g.ldx - 2) : (xc < g.M ? xc : g.M - 1);
  const int64_t xi1 = xc + 1 < g.M ? xc + 1 : g.M - 1;
  const int64_t yi0 = VEC ? (yc < g.ldy - 2 ? yc : g.ldy - 2) : (yc < g.N ? yc : g.N - 1);
  const int64_t yi1 = yc + 1 < g.N ? yc + 1 : g.N - 1;
  v2d xr[2], yr[2];
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t row = k0 + rg + 8 * i;
      row = row < ke ? row : ke - 1;
      xr[i] = load2<VEC>(X + row * g.ldx, xi0, xi1);
      yr[i] = load2<VEC>(Y + row * g.ldy, yi0, yi1);
    }
  };
  auto sstore = [&](int buf, int64_t k0) {
    double *Xs = smem + buf * STAGE_S;
    double *Ys = Xs + BK * LDS_S;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = rg + 8 * i;
      const bool rok = k0 + row < ke;
      v2d xv, yv;
      xv.x = (rok && x0ok) ? xr[i].x : 0.0;
      xv.y = (rok && x1ok) ? xr[i].y : 0.0;
      yv.x = (rok && y0ok) ? yr[i].x : 0.0;
      yv.y = (rok && y1ok) ? yr[i].y : 0.0;
      *reinterpret_cast<v2d *>(Xs + row * LDS_S + c2) = xv;
      *reinterpret_cast<v2d *>(Ys + row * LDS_S + c2) = yv;
    }
  };
  const int fr = lane & 15, fq = lane >> 4;
  if (kb < ke) {
    gload(kb);
    sstore(0, kb);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t k0 = kb; k0 < ke; k0 += BK) {
    const bool more = k0 + BK < ke;
    if (more) gload(k0 + BK);
    const double *Xs = smem + cur * STAGE_S;
    const double *Ys = Xs + BK * LDS_S;
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const int kr = kk * 4 + fq;
      double a[2], bb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = Xs[kr * LDS_S + wm * 32 + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < 2; ++j) bb[j] = Ys[kr * LDS_S + wn * 32 + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
    if (more) sstore(cur ^ 1, k0 + BK);
    __syncthreads();
    cur ^= 1;
  }
  const double alpha = g.alpha;
  const double beta = g.splits > 1 ? 0.0 : g.beta;
  double cv[2][2][4];
  if (beta != 0.0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t col = n0 + wn * 32 + j * 16 + fr;
          const int64_t row = m0 + wm * 32 + i * 16 + fq + 4 * r;
          const bool ok = col < g.N && row < g.M;
          cv[i][j][r] = C[(ok ? row : 0) * g.ldc + (ok ? col : 0)];
        }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = n0 + wn * 32 + j * 16 + fr;
      if (col >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + wm * 32 + i * 16 + fq + 4 * r;
        if (row >= g.M) continue;
        double v = alpha * acc[i][j][r];
        if (beta != 0.0) v += beta * cv[i][j][r];
        C[row * g.ldc + col] = v;
      }
    }
}

// 128 x 64-tile variant for IN-PLACE row panels (C aliases Y, M <= 128: the Cholesky row panel
// U[k, k+1:] = inv(U_kk)^T A[k, k+1:]): one workgroup still owns whole columns of the operand --
// which is what makes the in-place update safe -- but there are twice as many of them as with
// 128 x 128 tiles and each carries half the MFMA chain.  Single tile row only (blockIdx.x = tile
// column).  Same edge / triangular / beta / batch contract as the other kernels.
// PNW = 64, 32 or 16 columns per workgroup: late in a factorisation the panel has a handful of
// 64-column tiles for 256 CUs, and what it costs is the length of one workgroup's MFMA chain --
// narrower tiles spread the same columns over more CUs and shorten that chain.
constexpr int PN = 64;
constexpr int LDS_PX = BM + 16;   // 144
constexpr int LDS_PY = PN + 16;   // 80 (widest variant)
constexpr int STAGE_P = BK * (LDS_PX + LDS_PY);
constexpr size_t GEMM_LDS_BYTES_P = 2 * STAGE_P * sizeof(double);

// ---- one-shot row panel -----------------------------------------------------------------------
// The Cholesky row panel U[k, k+1:] = inv(U_kk)^T A[k, k+1:] at full tile size (M = K = 128, X upper
// triangular, in place) is latency, not work: 36 MFMAs per wave behind EIGHT dependent K stages of
// the kernel above (9.4 us at P = 4096, 35 launches per factorisation).  Here the whole inverse
// block (128 KiB, the same for every workgroup: L2 hits) and the workgroup's 16 operand columns go
// to LDS with ALL loads in flight at once -- one memory round trip -- then the MFMAs, balanced over
// the waves (16-row blocks i and 7 - i need 4 (i + 1) and 4 (8 - i) k-chunks of the triangle).
constexpr int OS_LDX = 136, OS_PN = 16;
constexpr size_t GEMM_LDS_BYTES_OS = (size_t)(128 * OS_LDX + 128 * OS_PN) * sizeof(double);

// X: row k = 1 KiB = one wave-instruction (lane -> 2 doubles); 32 rows per wave.  (Leaving the lanes
// left of the diagonal block out of the request -- half the bytes -- was measured: no gain.)
__device__ __forceinline__ void oneshot_stage_x(const double *X, int64_t ldx, double *Xs, int wave, int lane) {
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
#pragma unroll 8
  for (int i = 0; i < 32; ++i) {
    const int k = wave * 32 + i;
    __builtin_amdgcn_global_load_lds((glb_void *)(X + (int64_t)k * ldx + 2 * lane), (lds_void *)(Xs + k * OS_LDX), 16, 0, 0);
  }
}

// Y: 8 rows of 16 doubles per wave-instruction (lane -> row lane / 8, doubles 2 (lane % 8) ..)
__device__ __forceinline__ void oneshot_stage_y(const double *Yg, int64_t ldy, double *Ys, int wave, int lane) {
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k8 = (wave * 4 + i) * 8;
    __builtin_amdgcn_global_load_lds((glb_void *)(Yg + (int64_t)(k8 + (lane >> 3)) * ldy + 2 * (lane & 7)),
                                     (lds_void *)(Ys + k8 * OS_PN), 16, 0, 0);
  }
}

// this wave's two 16-row blocks (wave, 7 - wave) of inv(U_kk)^T Y: acc[r] <-> row 16 i + 4 r + lane / 16, column lane % 16
__device__ __forceinline__ void oneshot_product(const double *Xs, const double *Ys, int wave, int lane, v4d &acc0,
                                                v4d &acc1) {
  const int col = lane & 15, q = lane >> 4;
  const int i0 = wave, i1 = 7 - wave;
  acc0 = (v4d){0.0, 0.0, 0.0, 0.0};
  acc1 = (v4d){0.0, 0.0, 0.0, 0.0};
  const int n0c = 4 * (i0 + 1), n1c = 4 * (i1 + 1);
#pragma unroll 4
  for (int kc = 0; kc < n1c; ++kc) {
    const double bb = Ys[(4 * kc + q) * OS_PN + col];
    const double a1 = Xs[(4 * kc + q) * OS_LDX + 16 * i1 + col];
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bb, acc1, 0, 0, 0);
    if (kc < n0c) {
      const double a0 = Xs[(4 * kc + q) * OS_LDX + 16 * i0 + col];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bb, acc0, 0, 0, 0);
    }
  }
}

// one workgroup: 16 operand columns Yg[0..127][0..15] solved in place
__device__ __forceinline__ void oneshot_slice(const double *X, int64_t ldx, double *Yg, int64_t ldc, double *smem,
                                              int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  double *Xs = smem, *Ys = smem + 128 * OS_LDX;
  oneshot_stage_x(X, ldx, Xs, wave, lane);
  oneshot_stage_y(Yg, ldc, Ys, wave, lane);
  __syncthreads();   // (s_waitcnt vmcnt(0) is part of it)
  const int col = lane & 15, q = lane >> 4;
  const int i0 = wave, i1 = 7 - wave;            // this wave's two 16-row blocks of the output
  v4d acc0, acc1;
  oneshot_product(Xs, Ys, wave, lane, acc0, acc1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Yg[(int64_t)(16 * i0 + 4 * r + q) * ldc + col] = acc0[r];
    Yg[(int64_t)(16 * i1 + 4 * r + q) * ldc + col] = acc1[r];
  }
}

__global__ __launch_bounds__(256) void gemm_tn_f64_panel_oneshot_kernel(GemmDev g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.z;
  if (g.batch_active && !g.batch_active[b]) return;
  oneshot_slice(g.X + b * g.sx, g.ldx, g.C + b * g.sc + (int64_t)blockIdx.x * OS_PN, g.ldc, smem, threadIdx.x);   // C aliases Y
}

// ---- one-shot row panel of step k with the update of the next diagonal block riding along ------
// A[k+1, k+1] -= U[k, k+1]^T U[k, k+1] needs inv(U_kk) and the unsolved tile A[k, k+1] only, and both
// exist before this launch.  The first PD_PAIRS workgroups take one pair ti <= tj of 16-column blocks
// of tile k + 1 each: they solve slices tj and ti of a copy of A[k, k+1] that no panel workgroup
// overwrites (`pristine`, 128 x 128, row-major) with the panel's own product -- same operands, same
// order, the bits of the stored panel -- and wave 0 runs the 32-chunk chain of block (ti, tj) on
// them, exactly as the fused launch's workgroup 0 did (potf2_mfma.hip: diag_update_from_panel4, or
// diag_update_help4 + diag_update_collect4 for the nine helper blocks).  Redundant flops instead of
// a hand-off: no workgroup waits for another, the kernel boundary publishes the block.
// The other workgroups are the panel (oneshot_slice).
constexpr int PD_PAIRS = 36;

struct PanelDiagArgs {
  const double *X;          // inv(U_kk), 128 x 128, row-major
  double *Y;                // A[k, k+1 ..]: rest columns, solved in place
  int64_t ldc;
  const double *pristine;   // A[k, k+1] before the solve
  double *D;                // A[k+1, k+1] (ldc)
};

__global__ __launch_bounds__(256) void gemm_tn_f64_panel_oneshot_diag_kernel(PanelDiagArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (blockIdx.x >= PD_PAIRS) {
    oneshot_slice(g.X, CHOL_NB, g.Y + (int64_t)(blockIdx.x - PD_PAIRS) * OS_PN, g.ldc, smem, tid);
    return;
  }
  int ti = (int)blockIdx.x, tj = 0;     // pairs column by column: (0,0) (0,1) (1,1) (0,2) ...
  while (ti > tj) {
    ti -= tj + 1;
    ++tj;
  }
  const int col = lane & 15, q = lane >> 4;
  double *Xs = smem, *Ys = smem + 128 * OS_LDX;
  oneshot_stage_x(g.X, CHOL_NB, Xs, wave, lane);
  oneshot_stage_y(g.pristine + 16 * tj, CHOL_NB, Ys, wave, lane);
  v2d y2[4];                            // slice ti waits in registers for its turn in Ys (same lane mapping as the DMA)
  if (ti != tj) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k8 = (wave * 4 + i) * 8;
      y2[i] = *reinterpret_cast<const v2d *>(g.pristine + (int64_t)(k8 + (lane >> 3)) * CHOL_NB + 16 * ti + 2 * (lane & 7));
    }
  }
  v4d c = {0.0, 0.0, 0.0, 0.0};
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = g.D[(int64_t)(16 * ti + 4 * r + q) * g.ldc + 16 * tj + col];
  }
  __syncthreads();
  const int i0 = wave, i1 = 7 - wave;
  v4d acc0, acc1;
  double a[32], b[32];                  // wave 0: -u_ti and u_tj, k-chunk kc = rows 4 kc + q of the panel
  auto solved_to_lds = [&]() {          // the solved slice replaces the operand: the chain's one LDS hop
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Ys[(16 * i0 + 4 * r + q) * OS_PN + col] = acc0[r];
      Ys[(16 * i1 + 4 * r + q) * OS_PN + col] = acc1[r];
    }
    __syncthreads();
  };
  oneshot_product(Xs, Ys, wave, lane, acc0, acc1);
  solved_to_lds();
  if (wave == 0) {
#pragma unroll
    for (int kc = 0; kc < 32; ++kc) b[kc] = Ys[(4 * kc + q) * OS_PN + col];
  }
  if (ti != tj) {                       // (uniform over the workgroup)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k8 = (wave * 4 + i) * 8;
      *reinterpret_cast<v2d *>(Ys + (k8 + (lane >> 3)) * OS_PN + 2 * (lane & 7)) = y2[i];
    }
    __syncthreads();
    oneshot_product(Xs, Ys, wave, lane, acc0, acc1);
    solved_to_lds();
    if (wave == 0) {
#pragma unroll
      for (int kc = 0; kc < 32; ++kc) a[kc] = -Ys[(4 * kc + q) * OS_PN + col];
    }
  } else if (wave == 0) {
#pragma unroll
    for (int kc = 0; kc < 32; ++kc) a[kc] = -b[kc];
  }
  if (wave != 0) return;
  const bool helper = potf2_diag_helper_block(ti, tj);   // chain from zero, A added after it
  v4d acc = helper ? (v4d){0.0, 0.0, 0.0, 0.0} : c;
#pragma unroll
  for (int kc = 0; kc < 32; ++kc) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kc], b[kc], acc, 0, 0, 0);
  if (helper) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = c[r] + acc[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) g.D[(int64_t)(16 * ti + 4 * r + q) * g.ldc + 16 * tj + col] = acc[r];
}

bool panel_oneshot_diag_available() {
  static const bool ok = [] { const char *e = getenv("LSQAMD_PANEL_PN"); return !(e && atoi(e) != 0); }();
  return ok;
}

hipError_t launch_panel_oneshot_diag(hipStream_t st, const double *uinv, double *panel, int64_t lda, int64_t rest,
                                     const double *pristine, double *Dnext) {
  static PerDeviceOnce attr;
  const hipError_t ea = attr.run([] {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_f64_panel_oneshot_diag_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES_OS);
  });
  if (ea != hipSuccess) return ea;
  PanelDiagArgs g;
  g.X = uinv; g.Y = panel; g.ldc = lda; g.pristine = pristine; g.D = Dnext;
  hipLaunchKernelGGL(gemm_tn_f64_panel_oneshot_diag_kernel, dim3((unsigned)(PD_PAIRS + rest / OS_PN)), dim3(256),
                     GEMM_LDS_BYTES_OS, st, g);
  return hipGetLastError();
}

template <bool VEC, int PNW>
__global__ __launch_bounds__(256, 2) void gemm_tn_f64_panel_kernel(GemmDev g) {
  constexpr int WN = PNW >= 32 ? 2 : 1, WM = 4 / WN;       // waves along n / m
  constexpr int RW = BM / WM, NI = RW / 16;                  // rows per wave, 16-row blocks
  constexpr int CW = PNW / WN, NJ = CW / 16;                 // columns per wave, 16-column blocks
  constexpr int YT = PNW / 2, YROWS = 256 / YT;              // Y stage: column pairs, rows per pass
  constexpr int YP = (BK + YROWS - 1) / YROWS;               // passes over the 16 stage rows
  constexpr int LDY = PNW + 16;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = WN == 2 ? wave >> 1 : wave, wn = WN == 2 ? wave & 1 : 0;
  const int64_t m0 = 0, n0 = (int64_t)blockIdx.x * PNW;
  const int64_t b = blockIdx.z;
  if (g.batch_active && !g.batch_active[b]) return;
  const double *X = g.X + b * g.sx;
  const double *Y = g.Y + b * g.sy;
  double *C = g.C + b * g.sc;
  int64_t kb = 0, ke = g.K;
  if (g.x_upper_tri && ke > BM) ke = BM;
  v4d acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
  // X stage: 16 x 128 -> thread: column pair (tid & 63) * 2, rows (tid >> 6) + 4 i
  // Y stage: 16 x 64  -> thread: column pair (tid & 31) * 2, rows (tid >> 5) + 8 i
  const int xc2 = (tid & 63) * 2, xrg = tid >> 6;
  const int yc2 = (tid % YT) * 2, yrg = tid / YT;
  const int64_t xc = m0 + xc2, yc = n0 + yc2;
  const bool x0ok = xc < g.M, x1ok = xc + 1 < g.M;
  const bool y0ok = yc < g.N, y1ok = yc + 1 < g.N;
  const int64_t xi0 = VEC ? (xc < g.ldx - 2 ? xc : g.ldx - 2) : (xc < g.M ? xc : g.M - 1);
  const int64_t xi1 = xc + 1 < g.M ? xc + 1 : g.M - 1;
  const int64_t yi0 = VEC ? (yc < g.ldy - 2 ? yc : g.ldy - 2) : (yc < g.N ? yc : g.N - 1);
  const int64_t yi1 = yc + 1 < g.N ? yc + 1 : g.N - 1;
  v2d xr[4], yr[YP];
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t row = k0 + xrg + 4 * i;
      row = row < ke ? row : ke - 1;
      xr[i] = load2<VEC>(X + row * g.ldx, xi0, xi1);
    }
#pragma unroll
    for (int i = 0; i < YP; ++i) {
      int64_t row = k0 + yrg + YROWS * i;
      row = row < ke ? row : ke - 1;
      yr[i] = load2<VEC>(Y + row * g.ldy, yi0, yi1);
    }
  };
  auto sstore = [&](int buf, int64_t k0) {
    double *Xs = smem + buf * STAGE_P;
    double *Ys = Xs + BK * LDS_PX;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = xrg + 4 * i;
      const bool rok = k0 + row < ke;
      v2d xv;
      xv.x = (rok && x0ok) ? xr[i].x : 0.0;
      xv.y = (rok && x1ok) ? xr[i].y : 0.0;
      *reinterpret_cast<v2d *>(Xs + row * LDS_PX + xc2) = xv;
    }
#pragma unroll
    for (int i = 0; i < YP; ++i) {
      const int row = yrg + YROWS * i;
      if (row >= BK) continue;            // narrow variants: the upper thread rows have nothing to stage
      const bool rok = k0 + row < ke;
      v2d yv;
      yv.x = (rok && y0ok) ? yr[i].x : 0.0;
      yv.y = (rok && y1ok) ? yr[i].y : 0.0;
      *reinterpret_cast<v2d *>(Ys + row * LDY + yc2) = yv;
    }
  };
  const int fr = lane & 15, fq = lane >> 4;
  if (kb < ke) {
    gload(kb);
    sstore(0, kb);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t k0 = kb; k0 < ke; k0 += BK) {
    const bool more = k0 + BK < ke;
    if (more) gload(k0 + BK);
    const double *Xs = smem + cur * STAGE_P;
    const double *Ys = Xs + BK * LDS_PX;
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const int kr = kk * 4 + fq;
      double a[NI], bb[NJ];
#pragma unroll
      for (int i = 0; i < NI; ++i) a[i] = Xs[kr * LDS_PX + wm * RW + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bb[j] = Ys[kr * LDY + wn * CW + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
    if (more) sstore(cur ^ 1, k0 + BK);
    __syncthreads();
    cur ^= 1;
  }
  // every read of the operand columns this workgroup owns has happened (the loop's last barrier);
  // only now may C, which may alias Y, be written
  const double alpha = g.alpha, beta = g.beta;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t col = n0 + wn * CW + j * 16 + fr;
      if (col >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + wm * RW + i * 16 + fq + 4 * r;
        if (row >= g.M) continue;
        double v = alpha * acc[i][j][r];
        if (beta != 0.0) v += beta * C[row * g.ldc + col];
        C[row * g.ldc + col] = v;
      }
    }
}

static PerDeviceOnce g_attr_once;   // dynamic-LDS attributes of the product kernels, per device

static int64_t small_gemm_max() {
  static const int64_t v = [] {
    const char *e = getenv("LSQAMD_SMALL_GEMM_MAX");  // developer knob
    return e ? (int64_t)atoll(e) : (int64_t)600;
  }();
  return v;
}

static bool interior_eligible(const GemmTN &a) {
  const bool vx = !(a.ldx & 1) && !(reinterpret_cast<uintptr_t>(a.X) & 15) && !(a.sx & 1);
  const bool vy = !(a.ldy & 1) && !(reinterpret_cast<uintptr_t>(a.Y) & 15) && !(a.sy & 1);
  return vx && vy && (a.M % BM == 0) && (a.N % BN == 0) && (a.K % BK == 0) && !a.force_generic;
}

// few long tile rows (one large dense block: config 3's 8192 x 8192 W against 1024 columns is 32 row pairs x 8 tile
// columns = 256 workgroups, one per CU, four waves each with nothing to cover their barrier and LDS latencies):
// every tile row's K-range in two halves, 2x the workgroups, the second half into a scratch slab the caller adds.
bool gemm_tn_wants_tri_halves(const GemmTN &a) {
  const char *e = getenv("LSQAMD_TRI_HALVES");   // developer knob, read per call (A/B tests): 0 = one workgroup per tile-row pair
  const bool off = e && atoi(e) == 0;
  const int64_t tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
  const int64_t nwg = ((tiles_m + 1) / 2) * tiles_n * (a.batch < 1 ? 1 : a.batch);
  return !off && a.tri_halves && interior_eligible(a) && a.x_upper_tri && a.splits <= 1 && !a.work_map && tiles_m >= 8 &&
         nwg < 400 && a.split_stride != 0 && a.C != a.X && a.C != a.Y && !a.colsum_out;
}

static bool syrk_diag_off() {
  static const bool v = [] { const char *e = getenv("LSQAMD_SYRK_DIAG"); return e && atoi(e) == 0; }();  // developer knob
  return v;
}

bool gemm_tn_fuses_colsum(const GemmTN &a) {
  if (a.work_map) {
    // the split-K J^T J launch: diagonal tiles on the triangular schedule carry the column sums (<false, true, true>)
    const char *e = getenv("LSQAMD_SYRK_COLSUM");   // developer knob, read per call (A/B tests): 0 = separate J^T f pass
    const bool off = e && atoi(e) == 0;
    const int splits = a.splits < 1 ? 1 : a.splits;
    return interior_eligible(a) && !a.x_upper_tri && a.upper_only && a.X == a.Y && a.ldx == a.ldy && a.sx == a.sy &&
           a.M == a.N && (splits > 1 || a.beta == 0.0) && !syrk_diag_off() && !off && a.C != a.X;
  }
  // the conditions under which launch_gemm_tn reaches gemm_tn_f64_interior_kernel<true>
  const int64_t tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
  const int64_t nblk128 = tiles_m * tiles_n * (a.splits < 1 ? 1 : a.splits) * (a.batch < 1 ? 1 : a.batch);
  const bool small = !a.work_map && a.K <= 512 && nblk128 <= small_gemm_max();
  return interior_eligible(a) && a.x_upper_tri && a.splits <= 1 && !a.work_map && !small &&
         a.C != a.Y && a.C != a.X && a.alpha != 0.0;
}

hipError_t launch_gemm_tn(hipStream_t st, const GemmTN &a) {
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  {
    const hipError_t ea = g_attr_once.run([] {
      const void *fns[] = {reinterpret_cast<const void *>(gemm_tn_f64_kernel<true>),
                           reinterpret_cast<const void *>(gemm_tn_f64_kernel<false>),
                           reinterpret_cast<const void *>(gemm_tn_f64_interior_kernel<false, false>),
                           reinterpret_cast<const void *>(gemm_tn_f64_interior_kernel<false, true>),
                           reinterpret_cast<const void *>(gemm_tn_f64_interior_kernel<true, false>),
                           reinterpret_cast<const void *>(gemm_tn_f64_interior_kernel<false, true, true>),
                           reinterpret_cast<const void *>(gemm_tn_f64_interior_kernel<false, true, false, true>),
                           reinterpret_cast<const void *>(gemm_tn_f64_interior_kernel<false, true, true, true>)};
      for (const void *fn : fns) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    });
    if (ea != hipSuccess) return ea;
  }
  GemmDev g;
  g.X = a.X; g.Y = a.Y; g.C = a.C;
  g.M = a.M; g.N = a.N; g.K = a.K;
  g.ldx = a.ldx; g.ldy = a.ldy; g.ldc = a.ldc;
  g.alpha = a.alpha; g.beta = a.beta;
  g.sx = a.sx; g.sy = a.sy; g.sc = a.sc;
  g.vec_x = !((a.ldx & 1) || (reinterpret_cast<uintptr_t>(a.X) & 15) || (a.sx & 1));
  g.vec_y = !((a.ldy & 1) || (reinterpret_cast<uintptr_t>(a.Y) & 15) || (a.sy & 1));
  const int64_t tiles_m = (a.M + BM - 1) / BM;
  const int64_t tiles_n = (a.N + BN - 1) / BN;
  g.tiles_n = (int32_t)tiles_n;
  g.tiles_m = (int32_t)tiles_m;
  g.pair_rows = 0;
  g.tri_halves = 0;
  g.xcd_groups = 0;
  g.upper_only = a.upper_only;
  g.x_upper_tri = a.x_upper_tri;
  g.xy_lower_tri = a.xy_lower_tri;
  g.splits = a.splits < 1 ? 1 : a.splits;
  int64_t kchunk = (a.K + g.splits - 1) / g.splits;
  kchunk = (kchunk + BK - 1) / BK * BK;
  if (kchunk < BK) kchunk = BK;
  g.kchunk = kchunk;
  g.split_stride = g.splits > 1 ? a.split_stride : 0;
  g.work_map = a.work_map;
  g.n_work = a.n_work;
  const bool diag_off = syrk_diag_off();
  g.syrk_diag = a.work_map && a.X == a.Y && a.ldx == a.ldy && a.sx == a.sy && a.M == a.N &&
                (g.splits > 1 || a.beta == 0.0) && !diag_off;
  g.batch_active = a.batch_active;
  g.colsum_out = a.colsum_out;
  g.colsum_ld = a.colsum_ld;
  g.colsum_rcol = a.colsum_rcol;
  g.done_ctr = a.work_map ? a.done_ctr : nullptr;
  dim3 grid((unsigned)(tiles_m * tiles_n), (unsigned)g.splits, (unsigned)(a.batch < 1 ? 1 : a.batch));
  if (a.work_map) grid = dim3((unsigned)a.n_work, 1, (unsigned)(a.batch < 1 ? 1 : a.batch));
  const bool interior = g.vec_x && g.vec_y && (a.M % BM == 0) && (a.N % BN == 0) && (a.K % BK == 0) &&
                        !a.force_generic && !(a.x_upper_tri && a.work_map);  // no <XTRI, WORKMAP> instantiation
  // few tiles and a short K: latency-bound -> 64 x 64 tiles (4x the workgroups); threshold from a
  // sweep of potrf_upper at P = 4096 (160: 2.67 ms, 600: 2.56 ms, 1000: 2.56 ms)
  const int64_t nblk128 = tiles_m * tiles_n * g.splits * (a.batch < 1 ? 1 : a.batch);
  const int64_t small_max = small_gemm_max();
  // in-place products (C aliases an operand: the Cholesky row panel, the triangular inverse) are
  // only safe when ONE workgroup owns a whole column range of the operand, i.e. a single tile row
  const bool inplace = (a.C == a.Y) || (a.C == a.X);
  if (inplace && tiles_m > 1) return hipErrorInvalidValue;
  const bool small_ok = !inplace || a.M <= TS;
  if (inplace && a.C == a.Y && a.M > TS && a.K <= BM && g.splits == 1 && !a.force_generic) {
    // row panel: 128 x PNW tiles, one workgroup per PNW operand columns; PNW shrinks until there
    // are a few hundred workgroups (LSQAMD_PANEL_PN forces 64 / 32 / 16: developer knob)
    static const int force_pn = [] { const char *e = getenv("LSQAMD_PANEL_PN"); return e ? atoi(e) : 0; }();
    const int64_t nb_ = a.batch < 1 ? 1 : a.batch;
    if (force_pn == 0 && a.M == BM && a.K == BM && a.N % OS_PN == 0 && a.x_upper_tri && g.vec_x && g.vec_y &&
        a.alpha == 1.0 && a.beta == 0.0 && a.ldx >= BM) {
      static PerDeviceOnce attr_os;
      const hipError_t eo = attr_os.run([] {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_f64_panel_oneshot_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_LDS_BYTES_OS);
      });
      if (eo != hipSuccess) return eo;
      dim3 grido((unsigned)(a.N / OS_PN), 1, (unsigned)nb_);
      hipLaunchKernelGGL(gemm_tn_f64_panel_oneshot_kernel, grido, dim3(256), GEMM_LDS_BYTES_OS, st, g);
      return hipGetLastError();
    }
    int pn = (a.N * nb_ >= 200 * 64) ? 64 : ((a.N * nb_ >= 200 * 32) ? 32 : 16);
    if (force_pn == 64 || force_pn == 32 || force_pn == 16) pn = force_pn;
    g.tiles_n = (int32_t)((a.N + pn - 1) / pn);
    dim3 gridp((unsigned)g.tiles_n, 1, (unsigned)nb_);
    const bool vec = g.vec_x && g.vec_y;
#define LSQAMD_PANEL(V, W) hipLaunchKernelGGL((gemm_tn_f64_panel_kernel<V, W>), gridp, dim3(256), GEMM_LDS_BYTES_P, st, g)
    if (pn == 64) { if (vec) LSQAMD_PANEL(true, 64); else LSQAMD_PANEL(false, 64); }
    else if (pn == 32) { if (vec) LSQAMD_PANEL(true, 32); else LSQAMD_PANEL(false, 32); }
    else { if (vec) LSQAMD_PANEL(true, 16); else LSQAMD_PANEL(false, 16); }
#undef LSQAMD_PANEL
    return hipGetLastError();
  }
  // (... or ONE 64 x 64 tile whatever K is: J^T J for up to 64 parameters, where a 128 x 128 tile is three
  // quarters padding -- 0.33 -> 0.1 ms at N = 524288)
  const bool one_small_tile = a.M <= TS && a.N <= TS;
  if (!a.work_map && (a.K <= 512 || one_small_tile) && nblk128 <= small_max && !a.force_generic && small_ok) {
    const int64_t tm64 = (a.M + TS - 1) / TS, tn64 = (a.N + TS - 1) / TS;
    g.tiles_n = (int32_t)tn64;
    dim3 grid64((unsigned)(tm64 * tn64), (unsigned)g.splits, (unsigned)(a.batch < 1 ? 1 : a.batch));
    if (g.vec_x && g.vec_y)
      hipLaunchKernelGGL(gemm_tn_f64_small_kernel<true>, grid64, dim3(256), GEMM_LDS_BYTES_S, st, g);
    else
      hipLaunchKernelGGL(gemm_tn_f64_small_kernel<false>, grid64, dim3(256), GEMM_LDS_BYTES_S, st, g);
    return hipGetLastError();
  }
  if (interior && a.x_upper_tri) {
    if (tiles_m >= 4 && g.splits == 1 && !a.work_map) {  // balance the growing k-ranges (see kernel)
      g.pair_rows = 1;
      grid.x = (unsigned)(((tiles_m + 1) / 2) * tiles_n);
      if (gemm_tn_wants_tri_halves(a)) {
        g.tri_halves = 1;
        g.splits = 2;                       // (epilogue: beta ignored, split s -> C + s * split_stride)
        g.split_stride = a.split_stride;
        grid.y = 2;
      }
    }
    {
      static const bool xg_off = [] { const char *e = getenv("LSQAMD_XTRI_XCD_GROUPS"); return e && e[0] == '0'; }();   // developer knob
      const unsigned rows = grid.x / (unsigned)tiles_n, groups = rows * grid.y;
      if (!xg_off && !a.work_map && tiles_n >= 2 && groups % 8 == 0 && grid.x == rows * (unsigned)tiles_n) {
        g.xcd_groups = (int32_t)rows;
        grid.x = groups * (unsigned)tiles_n;
        grid.y = 1;
      }
    }
    hipLaunchKernelGGL((gemm_tn_f64_interior_kernel<true, false>), grid, dim3(256), GEMM_LDS_BYTES, st, g);
  }
  else if (interior && a.work_map && a.colsum_out) {
    if (!g.syrk_diag || !a.upper_only) return hipErrorInvalidValue;   // (callers ask gemm_tn_fuses_colsum first)
    if (g.done_ctr) hipLaunchKernelGGL((gemm_tn_f64_interior_kernel<false, true, true, true>), grid, dim3(256), GEMM_LDS_BYTES, st, g);
    else hipLaunchKernelGGL((gemm_tn_f64_interior_kernel<false, true, true>), grid, dim3(256), GEMM_LDS_BYTES, st, g);
  }
  else if (interior && a.work_map && g.done_ctr)
    hipLaunchKernelGGL((gemm_tn_f64_interior_kernel<false, true, false, true>), grid, dim3(256), GEMM_LDS_BYTES, st, g);
  else if (interior && a.work_map)
    hipLaunchKernelGGL((gemm_tn_f64_interior_kernel<false, true>), grid, dim3(256), GEMM_LDS_BYTES, st, g);
  else if (interior)
    hipLaunchKernelGGL((gemm_tn_f64_interior_kernel<false, false>), grid, dim3(256), GEMM_LDS_BYTES, st, g);
  else if (g.vec_x && g.vec_y)
    hipLaunchKernelGGL(gemm_tn_f64_kernel<true>, grid, dim3(256), GEMM_LDS_BYTES, st, g);
  else
    hipLaunchKernelGGL(gemm_tn_f64_kernel<false>, grid, dim3(256), GEMM_LDS_BYTES, st, g);
  return hipGetLastError();
}

// Work list for the upper-triangular tiles of a P x P SYRK with `splits` K-chunks:
// split-major, then 8 x 8 patches of tiles, then tiles of the patch.  Consecutive
// entries share row/column panels AND the K-chunk.  Within the run of entries each XCD walks (the
// kernel's blockIdx -> entry map: eight contiguous runs) the diagonal tiles go LAST: they take 10/16
// of the time of the others (triangular schedule), so the round of workgroups that drains each XCD
// is the short one.
int64_t syrk_work_count(int64_t P, int32_t splits) {
  const int64_t T = (P + BM - 1) / BM;
  return T * (T + 1) / 2 * (splits < 1 ? 1 : splits);
}

void syrk_work_fill(int64_t P, int32_t splits, int32_t *out) { (void)syrk_work_fill_rows(P, splits, 0, (int)((P + BM - 1) / BM), out); }

// the same list for the tile rows [row0, row1) only (the exchange groups of a sharded fit, eval.hip eval_normal_dev: one launch
// per group of tile rows, so that a group's packed tiles can be on their way to the other ranks while the next group is being
// computed); returns the number of entries.  Same ordering rules as the full list: 8 x 8 patches of tiles for the L2, one
// eighth of the list per XCD, a chunk's diagonal tiles last.
int64_t syrk_work_fill_rows(int64_t P, int32_t splits, int row0, int row1, int32_t *out) {
  const int T = (int)((P + BM - 1) / BM), PS = 8;
  const int NP = (T + PS - 1) / PS;
  if (row0 < 0) row0 = 0;
  if (row1 > T) row1 = T;
  int64_t o = 0;
  for (int s = 0; s < (splits < 1 ? 1 : splits); ++s)
    for (int pi = 0; pi < NP; ++pi)
      for (int pj = pi; pj < NP; ++pj)
        for (int tm = pi * PS; tm < (pi + 1) * PS && tm < T; ++tm) {
          if (tm < row0 || tm >= row1) continue;
          for (int tn = pj * PS; tn < (pj + 1) * PS && tn < T; ++tn) {
            if (tn < tm) continue;
            out[o++] = tm; out[o++] = tn; out[o++] = s; out[o++] = 0;
          }
        }
  const int64_t nw = o / 4, q = nw / 8, r = nw % 8;
  std::vector<int32_t> tmp;
  for (int xcd = 0; xcd < 8; ++xcd) {
    const int64_t b = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, n = q + (xcd < r ? 1 : 0);
    tmp.assign(out + 4 * b, out + 4 * (b + n));
    int64_t w = b;
    for (int keep = 0; keep < 2; ++keep)          // stable: off-diagonal entries, then diagonal ones
      for (int64_t e = 0; e < n; ++e)
        if ((tmp[4 * e] == tmp[4 * e + 1]) == (keep == 1)) {
          for (int c = 0; c < 4; ++c) out[4 * w + c] = tmp[4 * e + c];
          ++w;
        }
  }
  return nw;
}

// ONE list for ONE launch whose entries finish group by group: every XCD's run of the list (the kernel's blockIdx -> entry
// map: eight contiguous runs) holds its share of group 0 first, then of group 1, ... -- so all of group 0's tiles are in their
// slabs when about count[0] / total of the launch has run, and their exchange can start while the rest is computed.
// rows[g] .. rows[g + 1]: the tile rows of group g.  The 4th word of an entry is its group + 1; count[g] = entries of group g.
void syrk_work_fill_grouped(int64_t P, int32_t splits, int G, const int32_t *rows, int32_t *out, int32_t *count) {
  const int64_t nw = syrk_work_count(P, splits), q = nw / 8, r = nw % 8;
  std::vector<std::vector<int32_t>> lists((size_t)G);
  for (int g = 0; g < G; ++g) {
    lists[(size_t)g].resize(4 * (size_t)nw);
    // (rows-only fill WITHOUT its per-XCD diagonal-last pass: that pass is applied per (XCD run, group) segment below)
    const int T = (int)((P + BM - 1) / BM), PS = 8, NP = (T + PS - 1) / PS;
    int64_t o = 0;
    int32_t *L = lists[(size_t)g].data();
    for (int s = 0; s < (splits < 1 ? 1 : splits); ++s)
      for (int pi = 0; pi < NP; ++pi)
        for (int pj = pi; pj < NP; ++pj)
          for (int tm = pi * PS; tm < (pi + 1) * PS && tm < T; ++tm) {
            if (tm < rows[g] || tm >= rows[g + 1]) continue;
            for (int tn = pj * PS; tn < (pj + 1) * PS && tn < T; ++tn) {
              if (tn < tm) continue;
              L[o++] = tm; L[o++] = tn; L[o++] = s; L[o++] = g + 1;
            }
          }
    lists[(size_t)g].resize((size_t)o);
    count[g] = (int32_t)(o / 4);
  }
  // shares: group g gives XCD x  c[g][x] entries, sum_x = count[g], sum_g = the run length the kernel computes for x
  std::vector<int64_t> cap(8), pos((size_t)G, 0);
  for (int x = 0; x < 8; ++x) cap[(size_t)x] = q + (x < r ? 1 : 0);
  std::vector<std::vector<int64_t>> c((size_t)G, std::vector<int64_t>(8, 0));
  for (int g = 0; g < G; ++g) {
    if (g == G - 1) {
      for (int x = 0; x < 8; ++x) c[(size_t)g][(size_t)x] = cap[(size_t)x];
      break;
    }
    int64_t left = count[g];
    for (int x = 0; x < 8; ++x) {
      int64_t v = count[g] / 8;
      if (v > cap[(size_t)x]) v = cap[(size_t)x];
      c[(size_t)g][(size_t)x] = v;
      cap[(size_t)x] -= v;
      left -= v;
    }
    while (left > 0) {            // the remainder to the runs with the most room
      int best = 0;
      for (int x = 1; x < 8; ++x)
        if (cap[(size_t)x] > cap[(size_t)best]) best = x;
      c[(size_t)g][(size_t)best]++;
      cap[(size_t)best]--;
      --left;
    }
  }
  int64_t w = 0;
  for (int x = 0; x < 8; ++x)
    for (int g = 0; g < G; ++g) {
      const int32_t *L = lists[(size_t)g].data() + 4 * pos[(size_t)g];
      const int64_t n = c[(size_t)g][(size_t)x];
      for (int keep = 0; keep < 2; ++keep)          // stable: off-diagonal entries, then diagonal ones
        for (int64_t e = 0; e < n; ++e)
          if ((L[4 * e] == L[4 * e + 1]) == (keep == 1)) {
            for (int k = 0; k < 4; ++k) out[4 * w + k] = L[4 * e + k];
            ++w;
          }
      pos[(size_t)g] += n;
    }
}

// one wave waits until *ctr >= expect (acquire); gives up after ~4 s of wall clock and says so in *timed_out
__global__ __launch_bounds__(64) void wait_counter_kernel(const int32_t *ctr, int32_t expect, int32_t *timed_out) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();     // 100 MHz
  // poll RELAXED (an acquire per poll would invalidate this CU's L1 -- and cost the product beside it -- every time); the
  // kernels queued behind this one on the stream start with clean caches: the kernel boundary is their acquire
  while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < expect) {
    __builtin_amdgcn_s_sleep(64);
    if (__builtin_amdgcn_s_memrealtime() - t0 > 400000000ull) {
      __hip_atomic_store(timed_out, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
  }
}

hipError_t launch_wait_counter(hipStream_t st, const int32_t *ctr, int32_t expect, int32_t *timed_out) {
  hipLaunchKernelGGL(wait_counter_kernel, dim3(1), dim3(64), 0, st, ctr, expect, timed_out);
  return hipGetLastError();
}

// ---- whitening product with the raw Jacobian rows synthesised in LDS ---------------------------------
// J_b = W_b x Jraw_b for the sum models, the Y operand (16 raw rows x 128 columns per stage) computed
// by the workgroup instead of being read: the raw Jacobian (2.15 GB at the named shape) is neither
// written nor re-read.  Same tile, staging order and MFMA sequence as
// gemm_tn_f64_interior_kernel<true, false> -- the whitened rows come out bit-identical to the
// two-kernel route -- with the 128 tile columns = 64 terms k and their 64 partners K + k
// (value columns and frequency / exponent columns of the same terms share the sincos / exp):
//   thread t: term c = t & 63, stage rows t >> 6, + 4, + 8, + 12  ->  4 transcendental pairs per stage.
// fp64 VALU and fp64 MFMA share the datapath, so this work adds to the MFMA time (about a quarter)
// instead of hiding behind it; what is saved is the Jacobian kernel and 4.3 GB of traffic.
// NT = terms per tile: 64 (128 output columns) or 32 (64 output columns: twice the workgroups for the shapes
// that would otherwise leave one workgroup per CU -- config 3's single 8192-row block -- where nothing but
// a second workgroup covers the barrier and LDS latencies of the first); same products in the same order.
template <int MODEL, int NT, bool FAR>
__global__ __launch_bounds__(256, 2) void whiten_synth_kernel(WhitenSynth a, int tiles_m, int tiles_n, int pair_rows) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (a.trig_far && (a.trig_far[0] != 0) != FAR) return;    // (FAR = false: no far-range trig code, see model.hip)
  const int tid = threadIdx.x;
  // (wave made uniform: the staging destinations and the strip tests of the triangular stages are scalar.  A uniform value
  // alone does not make a branch scalar: while the skips compared 64-bit k indices they were vector compares and vcc
  // branches -- the scalar unit has no ordered 64-bit compare -- which is why mfmas_tri below tests a 32-bit stage index.)
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tm_first = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
  // pair_rows (blocks of many tile rows: the k-range of a tile row grows with it): this workgroup does tile
  // rows tm and tiles_m - 1 - tm one after the other, so that every workgroup sees the same total K
  const int npass = (pair_rows && tiles_m - 1 - tm_first != tm_first) ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
  if (pass == 1) __syncthreads();
  const int tm = pass == 0 ? tm_first : tiles_m - 1 - tm_first;
  const int64_t b = blockIdx.z;
  const int64_t m0 = (int64_t)tm * BM;
  const double *Xb = a.Wt + b * a.B * a.B;
  const double *xrow = a.x + b * a.B;
  double *C = a.J + b * a.B * a.ld;
  constexpr int NJ = NT / 16;                      // 16-column MFMA tiles per wave
  constexpr int SR = 256 / NT, NS = BK / SR;       // stage rows synthesised per pass of the workgroup, passes
  const int sc = tid % NT, srow = tid / NT;        // synthesis: term within the tile, first stage row
  const double amp = a.p[(int64_t)tn * NT + sc], frq = a.p[a.K + (int64_t)tn * NT + sc];

  v4d acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  const char *xb = reinterpret_cast<const char *>(Xb + (int64_t)wave * a.B + m0);
  const int64_t xstep = 4 * a.B * (int64_t)sizeof(double);
  uint32_t lane_off = 16u * (uint32_t)lane;
  // abscissae of the stage rows: a ring of three 32-double slots in LDS, slot s % 3 = x[16 s .. 16 s + 31],
  // filled two stages ahead by one 256-byte DMA of wave 0 -- no register ever waits on a global load in
  // the loop (vmcnt retires in order: a wait for x would be a wait for the operand rows behind it)
  double *xring = smem + 2 * STAGE;
  auto xdma = [&](int sidx) {
    if (wave == 0) {
      int64_t e = (int64_t)sidx * BK + (lane >> 1);
      if (e > a.B - 1) e = a.B - 1;
      const char *src = reinterpret_cast<const char *>(xrow + e) + 4 * (lane & 1);
      __builtin_amdgcn_global_load_lds((glb_void *)src, (lds_void *)(xring + (sidx % 3) * 32), 4, 0, 0);
    }
  };
  int ssyn = 0;         // index of the stage `stage_synth` builds next
  // (uniform row base + 32-bit lane offset, as in gemm_tn_f64_interior_kernel: see the comment at its staging lambda)
  auto stage_dma = [&](auto buf_tag) {
    constexpr int buf = decltype(buf_tag)::value;
    asm volatile("" : "+v"(lane_off));
    double *Xs = smem + buf * STAGE + wave * LDT;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((glb_void *)(xb + i * xstep + lane_off), (lds_void *)(Xs + 4 * i * LDT), 16, 0, 0);
    xb += 4 * xstep;
  };
  auto stage_synth = [&](auto buf_tag) {
    constexpr int buf = decltype(buf_tag)::value;
    double xs4[NS];
    const double *xq = xring + (ssyn % 3) * 32 + srow;
#pragma unroll
    for (int i = 0; i < NS; ++i) xs4[i] = xq[SR * i];
    double *Ys = smem + buf * STAGE + BK * LDT;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int row = srow + SR * i;
      const double xv = xs4[i];
      double t, dq;
      if (MODEL == LSQAMD_MODEL_COSMIX) {
        double sn, cs;
        sincos_moderate<FAR>(frq * xv, &sn, &cs);
        t = cs;
        dq = -amp * xv * sn;
      } else {
        const double e = exp(-frq * xv);
        t = e;
        dq = -amp * xv * e;
      }
      Ys[row * LDT + sc] = t;
      Ys[row * LDT + NT + sc] = dq;
    }
    ++ssyn;
  };
  const double wreg = (tid < BM) ? C[(m0 + tid) * a.ld + 2 * a.K] : 0.0;   // whitened residual of this tile's rows
  const int fr = lane & 15, fq = lane >> 4;
  using c0_tag = std::integral_constant<int, 0>;
  using c1_tag = std::integral_constant<int, 1>;
  xdma(0);
  xdma(1);
  stage_dma(c0_tag{});   // the first operand rows travel together with the abscissae: one exposed latency, not two
  __syncthreads();
  stage_synth(c0_tag{});
  __syncthreads();
  // A K stage out of buffer `cur` (a compile-time value: LDS addresses are base register + immediate) is `next`, the DMA
  // and the synthesis of the stage after it into the other buffer, then the MFMAs, then the barrier.
  const int nst = 8 * (tm + 1);
  auto next = [&](auto cur_tag, const int sidx) {
    constexpr int cur = decltype(cur_tag)::value;
    if (sidx + 1 < nst) {
      if (sidx + 2 < nst) xdma(sidx + 2);
      stage_dma(std::integral_constant<int, cur ^ 1>{});
      stage_synth(std::integral_constant<int, cur ^ 1>{});
    }
  };
  // full stage (k0 + BK <= m0): every strip takes every k-step
  auto mfmas_full = [&](auto cur_tag) {
    constexpr int cur = decltype(cur_tag)::value;
    const double *Xs = smem + cur * STAGE;
    const double *Ys = Xs + BK * LDT;
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const int kr = kk * 4 + fq;
      double av[4], bb[NJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = Xs[kr * LDT + (2 * i + wm) * 16 + fr];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bb[j] = Ys[kr * LDT + wn * NT + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bb[j], acc[i][j], 0, 0, 0);
    }
  };
  // stage ts = 0..7 of the tile row's own 128 k-values, k0 = m0 + 16 ts.  X[k][m] = 0 for k > m: strip t = 2 i + wm (rows
  // m0 + 16 t .. + 15) sees nothing from k-steps k0 + 4 kk > m0 + 16 t + 15, i.e. it takes all four k-steps of the stage
  // when t >= ts and none otherwise.  One 32-bit test of uniform values per strip (a scalar compare and branch), the strip
  // as the outer loop: every accumulator still receives its k-steps in ascending order, so the sums are the same.
  auto mfmas_tri = [&](auto cur_tag, const int ts) {
    constexpr int cur = decltype(cur_tag)::value;
    const double *Xs = smem + cur * STAGE;
    const double *Ys = Xs + BK * LDT;
    double bb[BK / 4][NJ];
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk)
#pragma unroll
      for (int j = 0; j < NJ; ++j) bb[kk][j] = Ys[(kk * 4 + fq) * LDT + wn * NT + j * 16 + fr];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (2 * i + wm < ts) continue;
      double av[BK / 4];
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) av[kk] = Xs[(kk * 4 + fq) * LDT + (2 * i + wm) * 16 + fr];
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], bb[kk][j], acc[i][j], 0, 0, 0);
    }
  };
  // the 8 tm full stages, unrolled by two (an even count: buffers 0, 1), then the eight triangular stages
  const int nfull = 8 * tm;
  for (int s = 0; s < nfull; s += 2) {
    next(c0_tag{}, s);
    mfmas_full(c0_tag{});
    __syncthreads();
    next(c1_tag{}, s + 1);
    mfmas_full(c1_tag{});
    __syncthreads();
  }
  for (int t = 0; t < 8; t += 2) {
    next(c0_tag{}, nfull + t);
    mfmas_tri(c0_tag{}, t);
    __syncthreads();
    next(c1_tag{}, nfull + t + 1);
    mfmas_tri(c1_tag{}, t + 1);
    __syncthreads();
  }
  double *wcol = smem, *red = smem + 128;
  if (tid < BM) wcol[tid] = wreg;
  __syncthreads();
  // tile column (wn, j, fr)  ->  Jacobian column: the value half (wn = 0) or the partner half at K + ..
  const int64_t cbase = (wn ? a.K : 0) + (int64_t)tn * NT;
  double sj[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) sj[j] = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rloc = (2 * i + wm) * 16 + fq;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double w = wcol[rloc + 4 * r];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const double v = acc[i][j][r];
        C[(m0 + rloc + 4 * r) * a.ld + cbase + j * 16 + fr] = v;
        sj[j] += v * w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    sj[j] += __shfl_xor(sj[j], 16, 64);
    sj[j] += __shfl_xor(sj[j], 32, 64);
  }
  if (fq == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) red[wave * 64 + j * 16 + fr] = sj[j];
  }
  __syncthreads();
  if (wm == 0 && fq == 0) {
    double *out = a.colsum_out + (b * tiles_m + tm) * (2 * a.K) + cbase;
#pragma unroll
    for (int j = 0; j < NJ; ++j) out[j * 16 + fr] = red[wave * 64 + j * 16 + fr] + red[(wave + 2) * 64 + j * 16 + fr];
  }
  }  // pass
}

// (Round 4 measured a variant in which ONE eight-wave workgroup owns both tile rows of a 256-row block and synthesises every
// raw row once -- a third less transcendental work: bit-identical rows, config 4's whitening 1.908 ms against 1.679.  The
// 512-thread barrier per stage with nothing else resident on the CU costs more than the sincos saved.  Removed in round 5;
// the record is in DESIGN_HISTORY.md.)

bool whiten_synth_eligible(int32_t model, int64_t B, int64_t P) {
  const char *e = getenv("LSQAMD_FUSED_JACOBIAN");   // developer knob, read per call: 0 = never, 2 = also for large blocks
  const bool off = e && e[0] == '0', always = e && e[0] == '2';
  // Large blocks: every tile row of the block synthesises the raw rows below it again -- B / 256 times each on average.
  // From eight tile rows on, writing the raw Jacobian once (it stays in the last-level cache) and reading it back is the
  // faster route (config 3, one 8192-row block: 1.52 ms synthesised, 1.45 ms read, 1.1 ms read with split tile rows).
  return !off && (model == LSQAMD_MODEL_COSMIX || model == LSQAMD_MODEL_MULTIEXP) && B >= BM && B % BM == 0 &&
         (B < 8 * BM || always) && P % 128 == 0 && P >= 128;
}

constexpr size_t SYNTH_LDS_BYTES = GEMM_LDS_BYTES + 3 * 32 * sizeof(double);

template <int MODEL, int NT, bool FAR>
static hipError_t launch_whiten_synth_one(hipStream_t st, const WhitenSynth &a, dim3 grid, int tiles_m, int tiles_n, int pair) {
  static PerDeviceOnce attr;   // one per instantiation
  const hipError_t ea = attr.run([] {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(whiten_synth_kernel<MODEL, NT, FAR>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)SYNTH_LDS_BYTES);
  });
  if (ea != hipSuccess) return ea;
  hipLaunchKernelGGL((whiten_synth_kernel<MODEL, NT, FAR>), grid, dim3(256), SYNTH_LDS_BYTES, st, a, tiles_m, tiles_n, pair);
  return hipGetLastError();
}

template <int MODEL, int NT>
static hipError_t launch_whiten_synth_nt(hipStream_t st, const WhitenSynth &a, dim3 grid, int tiles_m, int tiles_n, int pair) {
  // cosine model with a range flag: the kernel without far-range trig code first, then the safe one -- the
  // device flag leaves exactly one of them with work
  if (MODEL == LSQAMD_MODEL_COSMIX && a.trig_far) {
    hipError_t e = launch_whiten_synth_one<MODEL, NT, false>(st, a, grid, tiles_m, tiles_n, pair);
    if (e != hipSuccess) return e;
  }
  return launch_whiten_synth_one<MODEL, NT, true>(st, a, grid, tiles_m, tiles_n, pair);
}

hipError_t launch_whiten_synth(hipStream_t st, const WhitenSynth &a0) {
  WhitenSynth a = a0;
  if (a.model != LSQAMD_MODEL_COSMIX) a.trig_far = nullptr;
  const int tiles_m = (int)(a.B / BM);
  // few large blocks: unpaired, the workgroups of the last tile rows run 2 tiles_m / (tiles_m + 1) times the average
  const int pair = tiles_m >= 4 ? 1 : 0;
  const int64_t rows = pair ? (tiles_m + 1) / 2 : tiles_m;
  // 64 terms per tile unless that leaves the chip with (about) one workgroup per CU
  static const int64_t narrow_below = [] { const char *e = getenv("LSQAMD_SYNTH_NARROW"); return e ? atoll(e) : (int64_t)400; }();
  const bool narrow = rows * (a.K / 64) * a.nb < narrow_below && a.K % 32 == 0;
  const int tiles_n = (int)(a.K / (narrow ? 32 : 64));
  dim3 grid((unsigned)(rows * tiles_n), 1, (unsigned)a.nb);
  if (a.model == LSQAMD_MODEL_COSMIX)
    return narrow ? launch_whiten_synth_nt<LSQAMD_MODEL_COSMIX, 32>(st, a, grid, tiles_m, tiles_n, pair)
                  : launch_whiten_synth_nt<LSQAMD_MODEL_COSMIX, 64>(st, a, grid, tiles_m, tiles_n, pair);
  return narrow ? launch_whiten_synth_nt<LSQAMD_MODEL_MULTIEXP, 32>(st, a, grid, tiles_m, tiles_n, pair)
                : launch_whiten_synth_nt<LSQAMD_MODEL_MULTIEXP, 64>(st, a, grid, tiles_m, tiles_n, pair);
}

}  // namespace lsqamd

#ifdef LSQAMD_SYRK_STAMPS
extern "C" int lsqamd_debug_set_syrk_stamps(void *dev_ptr) try {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(lsqamd::g_syrk_stamps), &dev_ptr, sizeof(void *));
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)
#endif
