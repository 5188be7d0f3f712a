// The layout of a handle (host code only, gfx950 build): how the caller's one device workspace is sized and carved (carve,
// with the K-split of the J^T J product chosen by choose_splits), how the work list of that product is cut into the exchange
// groups of a sharded fit (plan_exchange_groups), the checks of a configuration and of what a handle must have been given
// before it runs (check_cfg, device_ok, ready), and the handle's buffers as the model kernels take them (model_args).
#include <cstdint>
#include <cstdlib>

#include "host.h"

using namespace lsqamd;

namespace lsqamd_host {

static int32_t choose_splits(int64_t N, int64_t P) {
  if (const char *e = getenv("LSQAMD_SYRK_SPLITS")) {  // tuning override (developer knob)
    const int v = atoi(e);
    if (v >= 1 && v <= 64) return v;
  }
  const int64_t T = (P + 127) / 128;
  const int64_t tiles = T * (T + 1) / 2;
  // enough workgroups to fill the chip a few times over (>= 2048: four rounds of two per CU), K-chunks of
  // ~4096 rows when there are that many rows (tail balance: 16 chunks beat 8 at N = 65536), never below 256
  // rows, never more than 16 slabs.  Their read-back in finalize_pack grows with the count: at the 8-GPU
  // shard shape N = 8192, P = 4096 (528 tiles) the product itself takes 3.07 / 2.53 / 2.24 / 2.10 / 2.10 ms
  // with 1 / 2 / 3 / 4 / 8 chunks and the read-back 0.06 / 0.07 / 0.09 / 0.10 / 0.16 ms: four.
  int64_t s = (2048 + tiles - 1) / tiles;
  if (s < N / 4096) s = N / 4096;
  // (few tiles: chunks down to 64 rows -- at (4096, 256) three tiles times 16 chunks are 48 workgroups on 256 CUs and the
  // product takes 40 us; 64 chunks: 21 us, the longer read-back of the slabs included in the balance below)
  const int64_t minrows = tiles <= 10 ? 64 : 256;
  const int64_t maxs = N / minrows > 1 ? N / minrows : 1;
  if (s > maxs) s = maxs;
  // ... except for FEW parameters and many rows (the usual shape of a fit): one or three tiles times 16 chunks
  // leaves 240 of the 256 CUs idle (N = 65536, P = 64: 0.62 ms for a product that reads 34 MB).  Slabs are
  // small there, so the count may grow to 256 as long as they stay within 64 MB together.
  const int64_t ldm = (P % 128 == 0) ? P + 128 : (P + 1 + 15) / 16 * 16;
  int64_t cap = (int64_t)(64 << 20) / (8 * P * ldm);
  if (cap > 256) cap = 256;
  if (cap < 16) cap = 16;
  if (s > cap) s = cap;
  // ... and for MANY rows at a few dozen tiles 16 chunks are one round of workgroups and a bit ((131072, 1024):
  // 576 workgroups, 2.81 ms; 32 chunks 2.26 ms): chunks of 4096 rows up to 32 of them, while the slabs stay
  // below a quarter of the Jacobian's own size
  int64_t more = N / 4096 < 32 ? N / 4096 : 32;
  const int64_t room = (N * P / 4) / (P * ldm);
  if (more > room) more = room;
  if (tiles >= 36 && s < more) s = more;
  if (s < 1) s = 1;
  return (int32_t)s;
}

size_t carve(lsqamd_fit *f, void *ws, size_t cap, bool dry) {
  const lsqamd_config &c = f->cfg;
  const int64_t N = c.n_data, P = c.n_param;
  f->N = N;
  f->P = P;
  f->ld = rup(P + 1, 16);
  // damped matrix [A | g | zero pad]: with P a multiple of 128 the pad makes every Cholesky
  // panel / trailing GEMM full-tile, so they run the direct-to-LDS interior kernel
  f->ldm = (P % 128 == 0) ? P + 128 : rup(P + 1, 16);
  f->ncols_aug = (P % 128 == 0) ? P + 128 : P + 1;
  f->npk = packed_doubles(P);
  f->splits = choose_splits(N, P);
  // row chunks of the two-stage J^T f: 256, more for many rows and few parameters (a chunk of 2048 rows is a
  // serial walk per thread: (524288, 64) took 0.25 ms for 268 MB) while the partial sums stay within 8 MB
  f->npartial = 256;
  while (f->npartial < 4096 && 2 * f->npartial <= N / 64 && 2 * f->npartial * (P + 1) * 8 <= (int64_t)(8 << 20))
    f->npartial *= 2;
  Carver cv(ws, cap, dry);
  f->x = cv.take<double>(N * (c.n_x > 0 ? c.n_x : 1));
  f->ymean = cv.take<double>(N);
  f->wdiag = cv.take<double>(N);
  f->in_block = cv.take<uint8_t>(N);
  f->row_param = cv.take<int32_t>(N);
  f->blk_row0 = cv.take<int64_t>(c.n_blocks);
  f->blk_size = cv.take<int64_t>(c.n_blocks);
  f->blk_woff = cv.take<int64_t>(c.n_blocks);
  f->wt = cv.take<double>(c.sum_block_sq);
  f->prior_mean = cv.take<double>(P);
  f->prior_prec = cv.take<double>(c.prior_dense ? P * P : P);
  f->p_dev = cv.take<double>(P);
  f->p_trial = cv.take<double>(P);
  f->p_buf0 = f->p_dev;
  f->r = cv.take<double>(N);
  f->r_raw = cv.take<double>(c.n_blocks > 0 ? N : 1);
  f->J = cv.take<double>(N * f->ld);
  f->Jraw = cv.take<double>(c.n_blocks > 0 ? N * f->ld : 1);
  f->slabs = cv.take<double>((int64_t)f->splits * P * f->ldm);
  f->redbuf = cv.take<double>(f->npk + P + 1);
  f->red_scalar = cv.take<double>(8);
  f->M = cv.take<double>(P * f->ldm);
  f->chol_work = cv.take<double>((int64_t)(potrf_work_bytes(P) / sizeof(double)));
  f->yv = cv.take<double>(4 * P + 8);   // y, v, then the hand-off granules of the chained back substitution
  f->diag_dev = cv.take<double>(P);
  f->dscale = cv.take<double>(P);
  f->tvec = cv.take<double>(P + 1);
  const int64_t part = f->npartial * (P + 1);
  f->partial = cv.take<double>(part > 2048 ? part : 2048);
  if (c.model == LSQAMD_MODEL_TAPE && P <= lsqamd_jit::NRM_MAX_P) f->nrm_part = cv.take<double>(NRM_BLOCKS * 96 + 128);
  f->Wl = cv.take<double>(P * f->ldm);
  f->cov = cv.take<double>(P * f->ldm);
  f->scal = cv.take<double>(16);
  f->lmd = cv.take<double>(LMS_COUNT);
  if (c.model == LSQAMD_MODEL_TAPE && P <= lsqamd_jit::FIT_MAX_P) f->fit_block = cv.take<double>(lsqamd_jit::FIT_HOST_DOUBLES);
  f->info_dev = cv.take<int32_t>(16);
  f->trig_far = cv.take<int32_t>(16);
  f->tape_cap = c.tape_len > 1024 ? c.tape_len : 1024;
  f->tape = cv.take<int32_t>(f->tape_cap);
  f->tape_poff = cv.take<int32_t>(f->tape_cap + 1);
  f->tape_seg = cv.take<int32_t>(3 * (int64_t)f->tape_cap + 3);
  f->consts = cv.take<double>(1024);
  if (c.model == LSQAMD_MODEL_TAPE) {
    // one forward + one reverse sweep per row: per resident wave 2 slots per instruction (upper
    // bound) x 64 lanes of local partial derivatives; at most 1024 waves are resident
    const int64_t groups = (N + 63) / 64;
    f->tape_wgs = (groups + 3) / 4 < 256 ? (groups + 3) / 4 : 256;
    if (f->tape_wgs < 1) f->tape_wgs = 1;
    f->tape_slot_cap = 2 * f->tape_cap;
    f->tape_part = cv.take<double>(f->tape_wgs * 4 * (int64_t)f->tape_slot_cap * 64);
    f->tape_ldn = rup(N > 0 ? N : 1, 64);
    f->tape_jt = cv.take<double>((P + 1) * f->tape_ldn);
  }
  f->syrk_nwork = (int32_t)syrk_work_count(P, f->splits);
  f->syrk_map = cv.take<int32_t>(4 * (int64_t)f->syrk_nwork);
  f->syrk_map_g = cv.take<int32_t>(4 * (int64_t)f->syrk_nwork);   // the same entries grouped by tile rows (grouped exchange)
  f->xg_ctr = cv.take<int32_t>(16);
  return cv.off;
}

int check_cfg(const lsqamd_config *c) {
  if (!c || c->abi_version != LSQAMD_ABI_VERSION) return LSQAMD_EINVAL;
  if (c->n_data < 0 || c->n_param < 1 || c->n_blocks < 0) return LSQAMD_EINVAL;
  if (c->model < LSQAMD_MODEL_COSMIX || c->model > LSQAMD_MODEL_IDENTITY) return LSQAMD_EINVAL;
  if (c->model == LSQAMD_MODEL_TAPE && c->n_param > LSQAMD_TAPE_MAX_PARAM) return LSQAMD_EINVAL;
  if (c->tape_len < 0 || c->tape_len > LSQAMD_TAPE_MAX_CODE) return LSQAMD_EINVAL;
  if ((c->model == LSQAMD_MODEL_COSMIX || c->model == LSQAMD_MODEL_MULTIEXP) && (c->n_param & 1))
    return LSQAMD_EINVAL;
  if (c->n_batch > 1) return LSQAMD_EUNSUPPORTED;
  return 0;
}

ModelArgs model_args(const lsqamd_fit *f, const double *p) {
  ModelArgs m;
  m.model = f->cfg.model;
  m.n_data = f->N;
  m.n_param = f->P;
  m.n_x = f->cfg.n_x > 0 ? f->cfg.n_x : 1;
  m.x = f->x;
  m.ymean = f->ymean;
  m.wdiag = f->wdiag;
  m.in_block = f->cfg.n_blocks > 0 ? f->in_block : nullptr;
  m.p = p;
  m.tape = f->tape;
  m.n_tape = f->n_tape;
  m.consts = f->consts;
  if (f->tape_part) {
    m.tape_poff = f->tape_poff;
    m.tape_part = f->tape_part;
    m.tape_jt = f->tape_jt;
    m.tape_ldn = f->tape_ldn;
    m.tape_wgs = f->tape_wgs;
    m.tape_slots = f->tape_slots;
    m.tape_seg = f->tape_seg;
    m.tape_n_seg = f->tape_n_seg;
    m.tape_seg_depth = f->tape_seg_depth;
    m.tape_seg_slots = f->tape_seg_slots;
    m.tape_single = f->tape_single;
    m.tape_slot_cap = f->tape_slot_cap;
  }
  m.jit = f->jit;
  if (!f->progs.empty()) {
    m.progs = f->progs.data();
    m.n_prog = (int32_t)f->progs.size();
  }
  return m;
}

// the library does not switch devices: the device that was current at lsqamd_create must be current in the calling thread
// (a launch on a stream of another device fails -- or, worse, a recycled block of another device is touched)
int device_ok(lsqamd_fit *f) {
  const int dev = current_device();
  if (f->dev >= 0 && dev != f->dev)
    FAIL(f, LSQAMD_EINVAL, "this handle was created on device %d, the calling thread's current device is %d (hipSetDevice first)", f->dev, dev);
  return 0;
}

int ready(lsqamd_fit *f) {
  if (const int rc = device_ok(f)) return rc;
  if (!f->have_data) FAIL(f, LSQAMD_EINVAL, "lsqamd_set_data has not been called");
  if (f->cfg.has_prior && !f->have_prior) FAIL(f, LSQAMD_EINVAL, "lsqamd_set_prior has not been called");
  if (f->cfg.model != LSQAMD_MODEL_IDENTITY && !f->have_x) FAIL(f, LSQAMD_EINVAL, "lsqamd_set_x has not been called");
  if (f->cfg.model == LSQAMD_MODEL_TAPE && !f->have_tape) FAIL(f, LSQAMD_EINVAL, "lsqamd_set_tape has not been called");
  return 0;
}

// LSQAMD_EXCHANGE_GROUPS = G (default 1): groups of tile rows with (about) equal tile counts -- the last one holds
// LSQAMD_EXCHANGE_TAIL_PCT per cent of the tiles when given (its exchange is the one nothing can hide)
int plan_exchange_groups(lsqamd_fit *f, int32_t *wm) {
  const int T = (int)((f->P + 127) / 128);
  int G = 1;
  if (const char *e = getenv("LSQAMD_EXCHANGE_GROUPS")) G = atoi(e);
  if (G > 8) G = 8;
  if (G > T) G = T;
  if (G < 1 || f->P <= 64) G = 1;
  f->xg = G;
  if (G == 1) return 0;
  const int64_t total = (int64_t)T * (T + 1) / 2;
  double tail = 1.0 / G;
  if (const char *e = getenv("LSQAMD_EXCHANGE_TAIL_PCT")) {
    const double v = atof(e) / 100.0;
    if (v > 0.0 && v < 1.0) tail = v;
  }
  int row = 0;
  int64_t tiles = 0;
  f->xg_row[0] = 0;
  for (int g = 1; g < G; ++g) {
    const double want = (1.0 - tail) * g / (G - 1) * (double)total;
    while (row < T - (G - g) && (double)(tiles + (T - row) / 2) < want) { tiles += T - row; ++row; }
    if (row <= f->xg_row[g - 1]) { tiles += T - row; ++row; }      // every group holds at least one tile row
    // the work list walks 8 x 8 PATCHES of tiles (two row panels serve eight tiles each way in the L2): a group
    // boundary inside a patch row leaves 1 x 8 slivers on both sides -- measured + 5 % on the product at the shard
    // shape.  Snap to the nearest multiple of 8 tile rows where that keeps the groups distinct
    if (T >= 16) {
      int snapped = (row + 4) / 8 * 8;
      if (snapped <= f->xg_row[g - 1]) snapped = f->xg_row[g - 1] + 8;
      if (snapped > f->xg_row[g - 1] && snapped <= T - (G - g)) {
        while (row < snapped) { tiles += T - row; ++row; }
        while (row > snapped) { --row; tiles -= T - row; }
      }
    }
    f->xg_row[g] = row;
  }
  f->xg_row[G] = T;
  const char *mode = getenv("LSQAMD_EXCHANGE_MODE");
  f->xg_signal = !(mode && mode[0] == 's' && mode[1] == 'p');          // "split": one product launch per group
  int64_t o = 0;
  for (int g = 0; g < G; ++g) {
    const int r0 = f->xg_row[g];
    f->xg_tile[g] = (int64_t)r0 * T - (int64_t)r0 * (r0 - 1) / 2;
  }
  f->xg_tile[G] = total;
  if (f->xg_signal) {
    syrk_work_fill_grouped(f->P, f->splits, G, f->xg_row, wm, f->xg_count);
    for (int g = 0; g < G; ++g) o += f->xg_count[g];
    if (hipMemsetAsync(f->xg_ctr, 0, 16 * sizeof(int32_t), f->st) != hipSuccess) return LSQAMD_EHIP;
  } else {
    for (int g = 0; g < G; ++g) {
      f->xg_work[g] = (int32_t)o;
      o += syrk_work_fill_rows(f->P, f->splits, f->xg_row[g], f->xg_row[g + 1], wm + 4 * o);
    }
    f->xg_work[G] = (int32_t)o;
  }
  return o == f->syrk_nwork ? 0 : LSQAMD_EHIP;
}

}  // namespace lsqamd_host
