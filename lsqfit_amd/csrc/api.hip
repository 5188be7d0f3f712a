// The C ABI of the single-fit library (include/lsqfit_amd.h; gfx950 build, host code only): every extern "C" entry point --
// creation and the setters, lsqamd_init / _step / _finish / _run (gsl_multifit_nlinear_init + _driver as
// src/lsqfit/_gsl.pyx:676-677 runs them), the evaluation and getter calls, fit.p sensitivities (lsqamd_dpdy), chi2 at many
// points (lsqamd_chi2_points), the debug exports -- and the helpers only they use.  What they drive lives next door: the
// trust-region drivers in lm_driver.hip, the device evaluation blocks in eval.hip, the workspace layout in workspace.hip,
// the recycled runtime objects in pool.hip; shared declarations in host.h, the handle in fit_state.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "host.h"

using namespace lsqamd;
using namespace lsqamd_host;

namespace {

// ---- host inputs of small problems: staged through pinned memory, uploaded without a wait -------------------------------
// A pageable source makes hipMemcpyAsync + the synchronisation the caller's buffer needs cost 14-20 us per setter -- four of
// them were a fifth of a whole small fit.  Small inputs (<= 16 KB each, 64 KB between two drains of the stream) are copied
// into a pinned arena the handle owns and uploaded from there: the setter returns at once, the stream orders the rest.
struct Upload {
  lsqamd_fit *f;
  bool waited_for = false;      // something went the direct way: the caller must synchronise before it returns
  explicit Upload(lsqamd_fit *fit) : f(fit) {}
  static bool is_host(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return true; }   // unregistered host memory
    return a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged;
  }
  hipError_t operator()(void *dst, const void *src, size_t bytes, bool maybe_device = false) {
    constexpr size_t ARENA = 64 << 10, ONE = 16 << 10;
    if (bytes == 0) return hipSuccess;
    if (bytes <= ONE && (!maybe_device || is_host(src))) {
      if (!f->stage) {
        f->stage = static_cast<char *>(pinned_take(ARENA, &f->stage_bytes));
        f->stage_off = 0;
      }
      if (f->stage) {
        const size_t need = (bytes + 63) & ~(size_t)63;
        if (f->stage_off + need > f->stage_bytes) {       // arena full: drain the stream, start over
          hipError_t e = hipStreamSynchronize(f->st);
          if (e != hipSuccess) return e;
          f->stage_off = 0;
        }
        std::memcpy(f->stage + f->stage_off, src, bytes);
        hipError_t e = hipMemcpyAsync(dst, f->stage + f->stage_off, bytes, hipMemcpyHostToDevice, f->st);
        f->stage_off += need;
        return e;
      }
    }
    waited_for = true;
    return hipMemcpyAsync(dst, src, bytes, maybe_device ? hipMemcpyDefault : hipMemcpyHostToDevice, f->st);
  }
  hipError_t finish() { return waited_for ? hipStreamSynchronize(f->st) : hipSuccess; }
};

// did a wait of the grouped exchange give up? (bounded spin: never a hang)
int exchange_timeout_check(lsqamd_fit *f) {
  if (!(f->comm && f->xg > 1 && f->xg_signal)) return 0;
  int32_t to = 0;
  HIPCHK(f, hipMemcpyAsync(&to, f->xg_ctr + 8, sizeof to, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  if (to) FAIL(f, LSQAMD_EREDUCE, "grouped exchange: the wait for a group of J^T J tiles timed out (the sums of this fit are not to be trusted)");
  return 0;
}

}  // namespace

// =========================================================================================
extern "C" {

int lsqamd_abi_version(void) { return LSQAMD_ABI_VERSION; }

int lsqamd_query_devices(int32_t *count, int32_t index, char *arch, size_t cap, int64_t *hbm_bytes) try {
  if (!count) return LSQAMD_EINVAL;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;   // no driver / no GPU: zero devices
  *count = n;
  if (arch && cap) arch[0] = 0;
  if (hbm_bytes) *hbm_bytes = 0;
  if (index < 0 || index >= n) return 0;
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, index) != hipSuccess) return LSQAMD_EHIP;
  if (arch && cap) snprintf(arch, cap, "%s", pr.gcnArchName);
  if (hbm_bytes) *hbm_bytes = (int64_t)pr.totalGlobalMem;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

size_t lsqamd_workspace_bytes(const lsqamd_config *cfg) try {
  if (check_cfg(cfg) != 0) return 0;
  lsqamd_fit tmp;
  tmp.cfg = *cfg;
  return carve(&tmp, nullptr, 0, true);
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_create(const lsqamd_config *cfg, void *dev_workspace, size_t workspace_bytes, void *stream,
                  lsqamd_fit **out) try {
  if (!out) return LSQAMD_EINVAL;
  *out = nullptr;
  const int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!dev_workspace || (reinterpret_cast<uintptr_t>(dev_workspace) & 255)) return LSQAMD_EINVAL;
  lsqamd_fit *f = new (std::nothrow) lsqamd_fit;
  if (!f) return LSQAMD_ENOMEM;
  f->cfg = *cfg;
  f->st = reinterpret_cast<hipStream_t>(stream);
  f->st_used = true;
  f->dev = current_device();
  const size_t need = carve(f, dev_workspace, workspace_bytes, true);
  if (need > workspace_bytes) {
    delete f;
    return LSQAMD_ENOMEM;
  }
  carve(f, dev_workspace, workspace_bytes, false);
  f->opt.xtol = 1e-8; f->opt.gtol = 1e-10; f->opt.ftol = 1e-10;   // __init__.py:102, _gsl.pyx:595-596
  f->opt.maxit = 1000;
  f->opt.scaler = LSQAMD_SCALE_MORE;
  f->opt.solver = LSQAMD_SOLVER_CHOLESKY;
  f->opt.factor_up = 3.0;
  f->opt.factor_down = 2.0;
  f->opt.trs = LSQAMD_TRS_LM;
  f->opt.avmax = 0.75;
  {
    const size_t P1 = (size_t)f->P + 1;
    const size_t head = (5 * P1 + 8 + 15) / 16 * 16;     // (the two regions the device writes start on 128-byte lines)
    f->pin = static_cast<double *>(pinned_take(sizeof(double) * (head + LMS_COUNT + 1280), &f->pin_bytes));
    if (!f->pin) {
      delete f;
      return LSQAMD_ENOMEM;
    }
    f->pin_g = f->pin; f->pin_c = f->pin_g + P1; f->pin_v = f->pin_c + P1; f->pin_d = f->pin_v + P1;
    f->pin_x = f->pin_d + P1; f->pin_s = f->pin_x + P1; f->pin_lm = f->pin + head;
    f->pin_fit = f->pin_lm + LMS_COUNT;       // 1280 doubles: what the one-launch fit kernel publishes (jit.h FitArgs::pub)
    static_assert(lsqamd_jit::FIT_HOST_DOUBLES <= 1280, "pin_fit");
    for (int i = 0; i < LMS_COUNT; ++i) f->pin_lm[i] = 0.0;
    f->pin_fit[16] = 0.0;
  }
  if (hipMemsetAsync(f->in_block, 0, (size_t)(f->N > 0 ? f->N : 1), f->st) != hipSuccess) {
    delete f;
    return LSQAMD_EHIP;
  }
  if (hipMemsetAsync(f->M, 0, sizeof(double) * (size_t)(f->P * f->ldm), f->st) != hipSuccess) {
    delete f;
    return LSQAMD_EHIP;
  }
  {
    std::vector<int32_t> wm(4 * (size_t)f->syrk_nwork);
    syrk_work_fill(f->P, f->splits, wm.data());
    Upload up(f);     // (a local: staged through pinned memory when small, else waited for)
    if (up(f->syrk_map, wm.data(), wm.size() * sizeof(int32_t)) != hipSuccess || up.finish() != hipSuccess) {
      delete f;
      return LSQAMD_EHIP;
    }
    if (plan_exchange_groups(f, wm.data()) != 0 ||
        (f->xg > 1 && (up(f->syrk_map_g, wm.data(), wm.size() * sizeof(int32_t)) != hipSuccess || up.finish() != hipSuccess))) {
      delete f;
      return LSQAMD_EHIP;
    }
  }
  *out = f;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

int lsqamd_destroy(lsqamd_fit *fit) try {
  if (!fit) return 0;
  (void)hipStreamSynchronize(fit->st);
  resolve_timers(fit);
  delete fit;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

const char *lsqamd_last_error(const lsqamd_fit *fit) { return fit ? fit->err.c_str() : "null handle"; }

int lsqamd_set_x(lsqamd_fit *f, const double *x, int64_t n_rows, int32_t n_x) try {
  if (!f) return LSQAMD_EINVAL;
  if (!x || n_rows != f->N || n_x != (f->cfg.n_x > 0 ? f->cfg.n_x : 1))
    FAIL(f, LSQAMD_EINVAL, "set_x: expected %lld x %d", (long long)f->N, f->cfg.n_x);
  {
    Upload up(f);
    HIPCHK(f, up(f->x, x, sizeof(double) * n_rows * n_x));
    HIPCHK(f, up.finish());
  }
  f->drop_step_graphs();   // captured steps bake xmax (and the path choices behind have_x) in by value
  f->xmax = 0.0;
  for (int64_t i = 0; i < n_rows * n_x; ++i) {
    const double ax = std::fabs(x[i]);
    if (!(ax <= f->xmax)) f->xmax = ax;      // (NaN sticks: the flag then always says "far")
  }
  f->have_x = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

// stack discipline and operand ranges of one RPN program (host side)
static int validate_tape(lsqamd_fit *f, const int32_t *code, int32_t n_code, int32_t n_consts) {
  int sp = 0;
  for (int t = 0; t < n_code; ++t) {
    const int op = code[t] & 0xff, arg = code[t] >> 8;
    if (op == LSQAMD_OP_CONST) { if (arg < 0 || arg >= n_consts) FAIL(f, LSQAMD_EINVAL, "tape: bad const index"); ++sp; }
    else if (op == LSQAMD_OP_X) { if (arg < 0 || arg >= (f->cfg.n_x > 0 ? f->cfg.n_x : 1)) FAIL(f, LSQAMD_EINVAL, "tape: bad x index"); ++sp; }
    else if (op == LSQAMD_OP_P) { if (arg < 0 || arg >= f->P) FAIL(f, LSQAMD_EINVAL, "tape: bad parameter index"); ++sp; }
    else if (op >= LSQAMD_OP_ADD && op <= LSQAMD_OP_POW) { if (sp < 2) FAIL(f, LSQAMD_EINVAL, "tape: stack underflow"); --sp; }
    else if (op >= LSQAMD_OP_NEG && op <= LSQAMD_OP_LAST) { if (sp < 1) FAIL(f, LSQAMD_EINVAL, "tape: stack underflow"); }
    else FAIL(f, LSQAMD_EINVAL, "tape: unknown opcode %d", op);
    if (sp > LSQAMD_TAPE_MAX_STACK) FAIL(f, LSQAMD_EINVAL, "tape: stack deeper than %d", LSQAMD_TAPE_MAX_STACK);
  }
  if (sp != 1) FAIL(f, LSQAMD_EINVAL, "tape: must leave exactly one value");
  return 0;
}

int lsqamd_set_tape(lsqamd_fit *f, const int32_t *code, int32_t n_code, const double *consts,
                    int32_t n_consts) try {
  if (!f) return LSQAMD_EINVAL;
  f->drop_step_graphs();
  if (f->st_used) (void)hipStreamSynchronize(f->st);      // (work queued on this handle may still run the kernel about to be released)
  f->drop_jit();
  f->progs.clear();
  f->used_nrm = false;
  f->J_stale = false;
  if (!code || n_code < 1 || n_code > f->tape_cap || n_consts < 0 || n_consts > 1024)
    FAIL(f, LSQAMD_EINVAL, "set_tape: 1..%d instructions (lsqamd_config.tape_len), <= 1024 constants", f->tape_cap);
  {
    const int rcv = validate_tape(f, code, n_code, n_consts);
    if (rcv) return rcv;
  }
  {
    std::vector<int32_t> poff((size_t)n_code + 1);
    int32_t slots = 0;
    for (int t = 0; t < n_code; ++t) {
      poff[(size_t)t] = slots;
      slots += tape_slots_of_op(code[t] & 0xff);
    }
    poff[(size_t)n_code] = slots;
    f->tape_slots = slots;
    // Is the root a sum S_1 + S_2 + ... ?  The joining ADDs are the ones that take the stack from depth 2 to 1;
    // S_1 ends where the depth is 1 for the last time before the first of them.  Every segment must fit the
    // kernel's LDS store of local partials; otherwise (or if anything follows the last join) the whole-tape
    // kernel runs.
    std::vector<int32_t> seg;      // (first, last, sign) per segment
    {
      std::vector<int> depth_after((size_t)n_code);
      int d = 0;
      std::vector<int> joins;
      for (int t = 0; t < n_code; ++t) {
        const int op = code[t] & 0xff;
        if (op <= LSQAMD_OP_P) ++d;
        else if (op <= LSQAMD_OP_POW) {
          if ((op == LSQAMD_OP_ADD || op == LSQAMD_OP_SUB) && d == 2) joins.push_back(t);
          --d;
        }
        depth_after[(size_t)t] = d;
      }
      bool ok = !joins.empty() && joins.back() == n_code - 1;
      if (ok) {
        int split = -1;
        for (int t = joins[0] - 1; t >= 0; --t)
          if (depth_after[(size_t)t] == 1) { split = t; break; }
        ok = split >= 0 && split + 1 <= joins[0] - 1;
        if (ok) {
          seg.insert(seg.end(), {0, split, 1});
          for (size_t k = 0; k < joins.size(); ++k) {
            const int lo = k == 0 ? split + 1 : joins[k - 1] + 1, hi = joins[k] - 1;
            if (lo > hi) { ok = false; break; }
            seg.insert(seg.end(), {lo, hi, (code[joins[k]] & 0xff) == LSQAMD_OP_SUB ? -1 : 1});
          }
        }
      }
      int max_depth = 1, max_slots = 1;
      for (size_t k = 0; ok && k + 2 < seg.size(); k += 3) {
        const int nsl = poff[(size_t)seg[k + 1] + 1] - poff[(size_t)seg[k]];
        if (nsl > 32) ok = false;     // TAPE_SEG_SLOTS
        if (nsl > max_slots) max_slots = nsl;
        int sd = 0;                              // every segment is a complete expression of its own
        for (int t = seg[k]; ok && t <= seg[k + 1]; ++t) {
          const int op = code[t] & 0xff;
          if (op <= LSQAMD_OP_P) ++sd;
          else if (op <= LSQAMD_OP_POW) { if (sd < 2) ok = false; --sd; }
          else if (sd < 1) ok = false;
          if (sd > max_depth) max_depth = sd;
        }
        if (sd != 1) ok = false;
      }
      if (!ok) seg.clear();
      f->tape_seg_depth = max_depth + 1;         // (the reverse sweep pushes one adjoint before it pops)
      f->tape_seg_slots = max_slots;
      // a parameter read once has one contribution to its column: a plain store, no atomic; if that is true of
      // all of them and none is missing, the transposed Jacobian needs no zero fill either
      std::vector<int> uses((size_t)f->P, 0);
      for (int t = 0; t < n_code; ++t)
        if ((code[t] & 0xff) == LSQAMD_OP_P) ++uses[(size_t)(code[t] >> 8)];
      int most = 0, least = 1 << 30;
      for (int u : uses) { if (u > most) most = u; if (u < least) least = u; }
      f->tape_single = most <= 1 ? (least == 1 ? 2 : 1) : 0;
    }
    f->tape_n_seg = (int32_t)(seg.size() / 3);
    Upload up(f);
    HIPCHK(f, up(f->tape_poff, poff.data(), sizeof(int32_t) * (n_code + 1)));
    if (!seg.empty()) HIPCHK(f, up(f->tape_seg, seg.data(), sizeof(int32_t) * seg.size()));
    HIPCHK(f, up.finish());   // (poff, seg are locals: staged copies or a wait)
  }
  {
    Upload up(f);
    HIPCHK(f, up(f->tape, code, sizeof(int32_t) * n_code));
    if (n_consts > 0) HIPCHK(f, up(f->consts, consts, sizeof(double) * n_consts));
    HIPCHK(f, up.finish());
  }
  f->n_tape = n_code;
  f->have_tape = true;
  // the formula as straight-line code for gfx950 (hiprtc, cached by content); without it the interpreter
  // kernels above run -- lsqamd_debug_flags bit 3 says which
  f->jit_why.clear();
  f->jit = lsqamd_jit::compile_tape(code, n_code, consts, n_consts, (int)f->P, f->cfg.n_x > 0 ? f->cfg.n_x : 1, f->jit_why);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_tape_programs(lsqamd_fit *f, int32_t n_prog, const int64_t *row0, const int32_t *code,
                             const int32_t *code_off, const double *consts, int32_t n_consts) try {
  if (!f) return LSQAMD_EINVAL;
  f->drop_step_graphs();
  f->used_nrm = false;
  f->J_stale = false;
  if (f->cfg.model != LSQAMD_MODEL_TAPE) FAIL(f, LSQAMD_EINVAL, "set_tape_programs: the handle's model is not LSQAMD_MODEL_TAPE");
  if (n_prog < 1 || !row0 || !code || !code_off || n_consts < 0 || n_consts > 1024 || (n_consts > 0 && !consts))
    FAIL(f, LSQAMD_EINVAL, "set_tape_programs: n_prog >= 1, row0[n_prog + 1], code, code_off[n_prog + 1], <= 1024 constants");
  if (row0[0] != 0 || row0[n_prog] != f->N || code_off[0] != 0 || code_off[n_prog] < 1 || code_off[n_prog] > f->tape_cap)
    FAIL(f, LSQAMD_EINVAL, "set_tape_programs: the row ranges must tile 0..%lld and the programs hold 1..%d instructions in all "
                           "(lsqamd_config.tape_len)", (long long)f->N, f->tape_cap);
  std::vector<lsqamd::TapeProgram> progs((size_t)n_prog);
  for (int i = 0; i < n_prog; ++i) {
    if (row0[i + 1] < row0[i] || code_off[i + 1] <= code_off[i])
      FAIL(f, LSQAMD_EINVAL, "set_tape_programs: row0 must not decrease and every program needs at least one instruction");
    const int rcv = validate_tape(f, code + code_off[i], code_off[i + 1] - code_off[i], n_consts);
    if (rcv) return rcv;
    progs[(size_t)i].row0 = row0[i];
    progs[(size_t)i].n_rows = row0[i + 1] - row0[i];
    progs[(size_t)i].tape_off = code_off[i];
    progs[(size_t)i].n_tape = code_off[i + 1] - code_off[i];
  }
  HIPCHK(f, hipMemcpyAsync(f->tape, code, sizeof(int32_t) * code_off[n_prog], hipMemcpyHostToDevice, f->st));
  if (n_consts > 0)
    HIPCHK(f, hipMemcpyAsync(f->consts, consts, sizeof(double) * n_consts, hipMemcpyHostToDevice, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  // every formula compiled on its own (hiprtc, cached by content); one that cannot be runs through the
  // forward-mode interpreter kernel over its rows
  f->drop_jit();
  f->progs.clear();
  f->jit_why.clear();
  int compiled = 0;
  for (int i = 0; i < n_prog; ++i) {
    std::string why;
    progs[(size_t)i].jit = lsqamd_jit::compile_tape(code + code_off[i], progs[(size_t)i].n_tape, consts, n_consts, (int)f->P,
                                                    f->cfg.n_x > 0 ? f->cfg.n_x : 1, why);
    if (progs[(size_t)i].jit) ++compiled;
    else f->jit_why = why;
  }
  f->progs = std::move(progs);
  f->progs_compiled = compiled;
  f->n_tape = code_off[n_prog];
  f->tape_n_seg = 0;
  f->have_tape = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_data(lsqamd_fit *f, const double *ymean, const double *wdiag, int32_t n_blocks,
                    const int64_t *block_row0, const int64_t *block_size, const int64_t *block_modes,
                    const int32_t *block_tri, const double *wt) try {
  if (!f) return LSQAMD_EINVAL;
  f->drop_step_graphs();
  if (n_blocks != f->cfg.n_blocks) FAIL(f, LSQAMD_EINVAL, "set_data: n_blocks differs from the config");
  if (f->N > 0 && (!ymean || !wdiag)) FAIL(f, LSQAMD_EINVAL, "set_data: null ymean/wdiag");
  if (n_blocks > 0 && (!block_row0 || !block_size || !block_modes || !wt))
    FAIL(f, LSQAMD_EINVAL, "set_data: null block arrays with n_blocks = %d", n_blocks);
  const int64_t N = f->N;
  std::vector<uint8_t> inb((size_t)(N > 0 ? N : 1), 0);
  f->h_row0.assign(block_row0, block_row0 + n_blocks);
  f->h_size.assign(block_size, block_size + n_blocks);
  f->h_modes.assign(block_modes, block_modes + n_blocks);
  f->h_tri.assign(n_blocks, 0);
  f->h_woff.assign(n_blocks, 0);
  int64_t off = 0, prev_end = 0, maxb = 0;
  bool all_tri = true;
  f->uniform_blocks = n_blocks > 0;
  for (int b = 0; b < n_blocks; ++b) {
    const int64_t r0 = f->h_row0[b], B = f->h_size[b];
    if (B < 1 || r0 < prev_end || r0 + B > N || f->h_modes[b] < 0 || f->h_modes[b] > B)
      FAIL(f, LSQAMD_EINVAL, "set_data: block %d is not a valid ascending contiguous row range", b);
    prev_end = r0 + B;
    if (B > maxb) maxb = B;
    f->h_tri[b] = block_tri ? block_tri[b] : 0;
    f->h_woff[b] = off;
    off += B * B;
    for (int64_t i = 0; i < B; ++i) inb[(size_t)(r0 + i)] = 1;
    if (B != f->h_size[0] || r0 != f->h_row0[0] + b * f->h_size[0]) f->uniform_blocks = false;
    if (!f->h_tri[b]) all_tri = false;
  }
  f->uniform_tri = all_tri ? 1 : 0;  // mixed blocks run batched without the triangular shortcut
  if (off > f->cfg.sum_block_sq || maxb > f->cfg.max_block)
    FAIL(f, LSQAMD_EINVAL, "set_data: blocks exceed the sizes promised in the config");
  Upload up(f);
  if (N > 0) {
    HIPCHK(f, up(f->ymean, ymean, sizeof(double) * N));
    HIPCHK(f, up(f->wdiag, wdiag, sizeof(double) * N));
    HIPCHK(f, up(f->in_block, inb.data(), (size_t)N));
  }
  if (n_blocks > 0) {
    if (!wt) FAIL(f, LSQAMD_EINVAL, "set_data: null block weights");
    HIPCHK(f, up(f->blk_row0, f->h_row0.data(), sizeof(int64_t) * n_blocks));
    HIPCHK(f, up(f->blk_size, f->h_size.data(), sizeof(int64_t) * n_blocks));
    HIPCHK(f, up(f->blk_woff, f->h_woff.data(), sizeof(int64_t) * n_blocks));
    HIPCHK(f, up(f->wt, wt, sizeof(double) * off, true));   // host or device source
  }
  HIPCHK(f, up.finish());
  f->have_data = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_ymean(lsqamd_fit *f, const double *ymean) try {
  if (!f || !ymean) return LSQAMD_EINVAL;
  if (!f->have_data) FAIL(f, LSQAMD_EINVAL, "set_ymean: call lsqamd_set_data first");
  {
    Upload up(f);
    if (f->N > 0) HIPCHK(f, up(f->ymean, ymean, sizeof(double) * f->N));
    HIPCHK(f, up.finish());
  }
  f->have_cov = false;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_prior(lsqamd_fit *f, const double *mean, const double *prec) try {
  if (!f) return LSQAMD_EINVAL;
  if (!f->cfg.has_prior) FAIL(f, LSQAMD_EINVAL, "set_prior: the config says has_prior = 0");
  if (!mean || !prec) FAIL(f, LSQAMD_EINVAL, "set_prior: null argument");
  const int64_t P = f->P;
  {
    Upload up(f);
    HIPCHK(f, up(f->prior_mean, mean, sizeof(double) * P));
    HIPCHK(f, up(f->prior_prec, prec, sizeof(double) * (f->cfg.prior_dense ? P * P : P), true));   // host or device source
    HIPCHK(f, up.finish());
  }
  f->have_prior = true;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_options(lsqamd_fit *f, const lsqamd_options *opt) try {
  if (!f || !opt) return LSQAMD_EINVAL;
  if (opt->xtol < 0 || opt->gtol < 0 || opt->maxit < 0) FAIL(f, LSQAMD_EINVAL, "set_options: negative tolerance/maxit");
  if (opt->scaler < 0 || opt->scaler > LSQAMD_SCALE_MARQUARDT) FAIL(f, LSQAMD_EINVAL, "set_options: unknown scaler");
  if (opt->solver != LSQAMD_SOLVER_CHOLESKY && opt->solver != LSQAMD_SOLVER_QR) FAIL(f, LSQAMD_EINVAL, "set_options: unknown solver");
  if (!(opt->factor_up > 1.0) || !(opt->factor_down > 1.0)) FAIL(f, LSQAMD_EINVAL, "set_options: factors must exceed 1");
  if (opt->trs < LSQAMD_TRS_LM || opt->trs > LSQAMD_TRS_MINPACK_LM) FAIL(f, LSQAMD_EINVAL, "set_options: unknown trust-region method");
  f->opt = *opt;
  f->drop_step_graphs();   // tolerances, factors and the scaler are baked into the captured nodes
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

size_t lsqamd_qr_work_bytes(const lsqamd_fit *f) { return f ? qr_work_bytes(f) : 0; }

int lsqamd_set_qr_work(lsqamd_fit *f, void *dev_work, size_t work_bytes) try {
  if (!f) return LSQAMD_EINVAL;
  if (dev_work && work_bytes < qr_work_bytes(f)) FAIL(f, LSQAMD_ENOMEM, "set_qr_work: need %zu bytes", qr_work_bytes(f));
  f->qr_work = dev_work;
  f->qr_work_bytes = dev_work ? work_bytes : 0;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_qr_info(const lsqamd_fit *f, int32_t *passes, double *delta) try {
  if (!f) return LSQAMD_EINVAL;
  if (passes) *passes = f->qr_passes;
  if (delta) *delta = f->qr_delta;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

int lsqamd_set_bounds(lsqamd_fit *f, const double *lower, const double *upper) try {
  if (!f) return LSQAMD_EINVAL;
  if (!lower && !upper) {
    f->lb.clear();
    f->ub.clear();
    return 0;
  }
  const int64_t P = f->P;
  std::vector<double> lb(P, -INFINITY), ub(P, INFINITY);
  for (int64_t j = 0; j < P; ++j) {
    if (lower) lb[j] = lower[j];
    if (upper) ub[j] = upper[j];
    if (!(lb[j] < ub[j]))
      FAIL(f, LSQAMD_EINVAL, "set_bounds: each lower bound must be strictly less than each upper bound (parameter %lld)",
           (long long)j);
  }
  f->lb.swap(lb);
  f->ub.swap(ub);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_loss(lsqamd_fit *f, int32_t loss, double f_scale) try {
  if (!f) return LSQAMD_EINVAL;
  if (loss < LSQAMD_LOSS_LINEAR || loss > LSQAMD_LOSS_ARCTAN) FAIL(f, LSQAMD_EINVAL, "set_loss: `loss` must be linear, soft_l1, huber, cauchy or arctan");
  if (!(f_scale > 0.0) || !std::isfinite(f_scale)) FAIL(f, LSQAMD_EINVAL, "set_loss: f_scale must be positive");
  f->loss = loss;
  f->f_scale = f_scale;
  f->drop_step_graphs();
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_x_scale(lsqamd_fit *f, const double *x_scale) try {
  if (!f) return LSQAMD_EINVAL;
  std::vector<double> v;
  if (x_scale) {
    v.assign(x_scale, x_scale + f->P);
    for (int64_t j = 0; j < f->P; ++j)
      if (!(v[j] > 0.0) || !std::isfinite(v[j])) FAIL(f, LSQAMD_EINVAL, "set_x_scale: `x_scale` must be 'jac' or array_like with positive numbers");
  }
  f->x_scale.swap(v);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_param_rows(lsqamd_fit *f, const int32_t *row_param) try {
  if (!f) return LSQAMD_EINVAL;
  f->drop_step_graphs();
  if (!row_param) {
    f->have_param_rows = false;
    return 0;
  }
  if (f->cfg.has_prior) FAIL(f, LSQAMD_EINVAL, "set_param_rows: the prior is given as rows OR through lsqamd_set_prior, not both");
  bool any = false;
  for (int64_t i = 0; i < f->N; ++i) {
    if (row_param[i] >= f->P) FAIL(f, LSQAMD_EINVAL, "set_param_rows: row %lld names parameter %d", (long long)i, row_param[i]);
    any |= row_param[i] >= 0;
  }
  if (f->N > 0) {
    HIPCHK(f, hipMemcpyAsync(f->row_param, row_param, sizeof(int32_t) * f->N, hipMemcpyHostToDevice, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
  }
  f->have_param_rows = any;
  f->initialised = false;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_linear(lsqamd_fit *f, const int32_t *index, int32_t n) try {
  if (!f || n < 0 || (n > 0 && !index)) return LSQAMD_EINVAL;
  std::vector<char> mask;
  if (n > 0) {
    mask.assign(f->P, 0);
    for (int32_t k = 0; k < n; ++k) {
      if (index[k] < 0 || index[k] >= f->P) FAIL(f, LSQAMD_EINVAL, "set_linear: index %d out of range", index[k]);
      mask[index[k]] = 1;
    }
  }
  f->linear.swap(mask);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_set_reduce(lsqamd_fit *f, lsqamd_reduce_fn fn, void *user) try {
  if (!f) return LSQAMD_EINVAL;
  f->reduce = fn;
  f->reduce_user = user;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

// rank that contributes the (replicated) prior terms before the all-reduce; default: this one
int lsqamd_set_adds_prior(lsqamd_fit *f, int32_t on) try {
  if (!f) return LSQAMD_EINVAL;
  f->adds_prior = on != 0;
  f->drop_step_graphs();
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_init(lsqamd_fit *f, const double *p0) try {
  if (!f || !p0) return LSQAMD_EINVAL;
  return do_init(f, p0);
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_step(lsqamd_fit *f, int32_t *info) try {
  if (!f) return LSQAMD_EINVAL;
  if (const int rcd = device_ok(f)) return rcd;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "lsqamd_step before lsqamd_init");
  if (f->opt.trs >= LSQAMD_TRS_TRF) FAIL(f, LSQAMD_EUNSUPPORTED, "lsqamd_step: the scipy-plugin methods (trf, dogbox, minpack lm) run through lsqamd_run only");
  int met = 0;
  const int rc = driver_iteration(f, &met, true);
  if (rc < 0) return rc;
  if (f->timing) resolve_timers(f, true);
  if (info) *info = met;
  return rc;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_finish(lsqamd_fit *f, lsqamd_summary *out) try {
  if (!f) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "lsqamd_finish before lsqamd_init");
  const int rc = do_covariance(f);
  if (f->timing) resolve_timers(f);
  if (const int rcx = exchange_timeout_check(f)) return rcx;
  fill_summary(f, out, 0, 0);
  if (out) out->cov_status = rc == LSQAMD_ENOTPD ? rc : (rc == 0 && f->cov_inaccurate ? LSQAMD_EINACCURATE : (rc == 0 ? f->cov_dropped : 0));
  return rc == LSQAMD_ENOTPD ? 0 : rc;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

// After a fit with a robust loss (cov_rc: what its covariance came to).  That covariance is the loss-scaled Jacobian's, which
// scipy returns (src/lsqfit/_scipy.py:165-169); chi2 and log det(J^T J) -- and what the getters hand out from here on -- are
// those of the TRUE residuals and Jacobian at the fit point (:160-161, src/lsqfit/__init__.py:667,:719): one more
// evaluation, without the loss
static int true_residual_state(lsqamd_fit *f, int cov_rc) {
  const int32_t loss = f->loss;
  f->loss = LSQAMD_LOSS_LINEAR;
  int r2 = eval_normal_dev(f, f->p_dev, true);
  if (r2 == 0) r2 = logdet_normal(f);
  f->loss = loss;
  f->njev--;                      // (bookkeeping of the library, not an evaluation of the method)
  if (r2 < 0 && r2 != LSQAMD_ENOTPD) return r2;
  // (the evaluation above overwrote the loss-scaled normal matrix: the covariance in f->cov stays valid only if it was
  // made; a later lsqamd_get_cov must not recompute it from the UNSCALED matrix that is there now)
  f->have_cov = cov_rc == 0;
  f->cov_unavailable = cov_rc != 0;
  return 0;
}

// t_run_ms of a run that began at event a (cov_rc: what its covariance came to); frees the staging arena once nothing runs
static float run_elapsed_ms(lsqamd_fit *f, hipEvent_t a, hipEvent_t b, int cov_rc) {
  float ms = 0.f;
  if (f->used_one_launch && f->have_cov && cov_rc == 0) {
    // the whole run was the one kernel whose last word the host has already seen: nothing is left on the stream to wait for
    // (an event synchronisation is ~15 us of sleeping and waking); the kernel timed itself (100 MHz ticks)
    ms = (float)(f->fit_rec[(size_t)lsqamd_jit::fit_host_diag((int)f->P) + 4] * 1e-5);
    f->stage_off = 0;
  } else {
    (void)hipEventRecord(b, f->st);
    if (hipEventSynchronize(b) == hipSuccess) f->stage_off = 0;
    (void)hipEventElapsedTime(&ms, a, b);
  }
  return ms;
}

int lsqamd_run(lsqamd_fit *f, const double *p0, lsqamd_summary *out) try {
  if (!f || !p0) return LSQAMD_EINVAL;
  struct Pair {   // recycled events: every return path hands them back
    lsqamd_fit *f;
    hipEvent_t a, b;
    explicit Pair(lsqamd_fit *fit) : f(fit), a(take_event(fit)), b(take_event(fit)) {}
    ~Pair() { f->event_pool.push_back(a); f->event_pool.push_back(b); }
  } ev(f);
  (void)hipEventRecord(ev.a, f->st);
  f->used_one_launch = false;
  f->cov_host_valid = false;
  // the method from p0 to its end: one of scipy's three, the whole fit in one launch, or GSL's driver loop on the host
  int rc = 0, info = 0, status = -2;
  if (f->opt.trs >= LSQAMD_TRS_TRF) rc = run_scipy_method(f, p0, &status, &info);
  else if ((rc = run_one_launch(f, p0, &status, &info)) == 0) rc = run_gsl_driver(f, p0, &status, &info);
  else if (rc > 0) rc = 0;
  if (rc) return rc;
  rc = (f->used_one_launch && f->have_cov) ? 0 : do_covariance(f);
  if (rc < 0 && rc != LSQAMD_ENOTPD) return rc;
  if (f->robust()) {
    const int r2 = true_residual_state(f, rc);
    if (r2) return r2;
  }
  const float ms = run_elapsed_ms(f, ev.a, ev.b, rc);
  if (f->timing) resolve_timers(f);
  if (const int rcx = exchange_timeout_check(f)) return rcx;
  fill_summary(f, out, status, info);
  if (out) {
    out->t_run_ms = ms;
    // LSQAMD_ENOTPD: J^T J singular at the end point, cov / logdet undefined; LSQAMD_EINACCURATE: delivered, degraded
    out->cov_status = rc == 0 && f->cov_inaccurate ? LSQAMD_EINACCURATE : (rc == 0 ? f->cov_dropped : rc);
  }
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_eval_residual(lsqamd_fit *f, const double *p, double *chi2) try {
  if (!f || !p || !chi2) return LSQAMD_EINVAL;
  int rc = ready(f);
  if (rc) return rc;
  HIPCHK(f, hipMemcpyAsync(f->p_trial, p, sizeof(double) * f->P, hipMemcpyHostToDevice, f->st));
  rc = eval_residual_dev(f, f->p_trial, chi2);
  if (f->timing) resolve_timers(f);
  return rc;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_eval_fcn(lsqamd_fit *f, const double *p, double *out, size_t cap) try {
  if (!f || !p || !out) return LSQAMD_EINVAL;
  int rc = ready(f);
  if (rc) return rc;
  const int64_t N = f->N;
  if (cap < (size_t)N) FAIL(f, LSQAMD_ECAPACITY, "eval_fcn: need %lld", (long long)N);
  if (N == 0) return 0;
  // residual kernel: w (f - y) for the 1x1 rows, f - y for the rows inside blocks
  HIPCHK(f, hipMemcpyAsync(f->p_trial, p, sizeof(double) * f->P, hipMemcpyHostToDevice, f->st));
  ModelArgs m = model_args(f, f->p_trial);
  HIPCHK(f, launch_residual_ex(f->st, m, f->r, f->r_raw));
  if (f->have_param_rows)     // rows that ARE parameters (lsqamd_set_param_rows): their "function value" is p_j
    HIPCHK(f, launch_param_rows(f->st, f->row_param, f->N, f->P, 1, f->p_trial, f->ymean, f->wdiag,
                                f->cfg.n_blocks > 0 ? f->in_block : nullptr, f->r, f->r_raw, 0));
  std::vector<double> r((size_t)N), rr((size_t)N, 0.0), y((size_t)N), w((size_t)N);
  std::vector<uint8_t> inb((size_t)N, 0);
  HIPCHK(f, hipMemcpyAsync(r.data(), f->r, sizeof(double) * N, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(y.data(), f->ymean, sizeof(double) * N, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipMemcpyAsync(w.data(), f->wdiag, sizeof(double) * N, hipMemcpyDeviceToHost, f->st));
  if (f->cfg.n_blocks > 0) {
    HIPCHK(f, hipMemcpyAsync(rr.data(), f->r_raw, sizeof(double) * N, hipMemcpyDeviceToHost, f->st));
    HIPCHK(f, hipMemcpyAsync(inb.data(), f->in_block, (size_t)N, hipMemcpyDeviceToHost, f->st));
  }
  HIPCHK(f, hipStreamSynchronize(f->st));
  for (int64_t i = 0; i < N; ++i)
    out[i] = y[(size_t)i] + (inb[(size_t)i] ? rr[(size_t)i] : r[(size_t)i] / w[(size_t)i]);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_eval_normal(lsqamd_fit *f, const double *p, double *chi2) try {
  if (!f || !p) return LSQAMD_EINVAL;
  int rc = ready(f);
  if (rc) return rc;
  const int64_t P = f->P;
  f->hx.assign(p, p + P);
  f->hg.assign(P, 0.0);
  f->hcoln.assign(P, 0.0);
  f->hv.assign(P, 0.0);
  f->hdx.assign(P, 0.0);
  if ((int64_t)f->hdiag.size() != P) f->hdiag.assign(P, 1.0);
  f->dev_lm = false;
  f->mirrors_stale = false;
  HIPCHK(f, hipMemcpyAsync(f->p_dev, p, sizeof(double) * P, hipMemcpyHostToDevice, f->st));
  rc = eval_normal_dev(f, f->p_dev);
  if (f->timing) resolve_timers(f);
  if (rc) return rc;
  // the Jacobian evaluation leaves the whitened residual in column P of J; mirror it into r
  HIPCHK(f, launch_copy_strided(f->st, f->J + P, f->ld, f->r, 1, f->N, 1));
  f->initialised = true;
  if (chi2) *chi2 = f->chi2;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_solve_damped(lsqamd_fit *f, double mu, const double *diag, double *v) try {
  if (!f || !diag || !v) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "solve_damped needs lsqamd_eval_normal / lsqamd_init first");
  const int rc = solve_damped_dev(f, mu, diag);
  if (f->timing) resolve_timers(f);
  if (rc) {
    if (rc == LSQAMD_ENOTPD) f->err = "damped normal matrix is not positive definite";
    return rc;
  }
  std::memcpy(v, f->hv.data(), sizeof(double) * f->P);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_op_gemm_tn(void *stream, int64_t M, int64_t N, int64_t K, double alpha, const double *X,
                      int64_t ldx, const double *Y, int64_t ldy, double beta, double *C, int64_t ldc,
                      int32_t upper_only, int32_t x_upper_tri) try {
  GemmTN g;
  g.X = X; g.Y = Y; g.C = C;
  g.M = M; g.N = N; g.K = K;
  g.ldx = ldx; g.ldy = ldy; g.ldc = ldc;
  g.alpha = alpha; g.beta = beta;
  g.upper_only = upper_only;
  g.x_upper_tri = x_upper_tri;
  return launch_gemm_tn(reinterpret_cast<hipStream_t>(stream), g) == hipSuccess ? 0 : LSQAMD_EHIP;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

size_t lsqamd_op_potrf_work_bytes(int64_t n) { return potrf_work_bytes(n); }

int lsqamd_op_potrf_upper(void *stream, double *A, int64_t n, int64_t lda, int64_t n_cols, double *work,
                          size_t work_bytes, int32_t *dev_info) try {
  if (work_bytes < potrf_work_bytes(n)) return LSQAMD_ENOMEM;
  return potrf_upper(reinterpret_cast<hipStream_t>(stream), A, n, lda, n_cols, work, dev_info) == hipSuccess
             ? 0 : LSQAMD_EHIP;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

int64_t lsqamd_nf(const lsqamd_fit *f) try {
  if (!f) return 0;
  int64_t nf = f->N;
  for (size_t b = 0; b < f->h_size.size(); ++b) nf -= f->h_size[b] - f->h_modes[b];
  if (f->cfg.has_prior) nf += f->P;
  return nf;
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_get_x(lsqamd_fit *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (cap < (size_t)f->P) FAIL(f, LSQAMD_ECAPACITY, "get_x: need %lld", (long long)f->P);
  if ((int64_t)f->hx.size() != f->P) FAIL(f, LSQAMD_EINVAL, "get_x: no fit has run");
  if (const int rcm = refresh_mirrors(f)) return rcm;
  std::memcpy(out, f->hx.data(), sizeof(double) * f->P);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_get_grad(lsqamd_fit *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (cap < (size_t)f->P) FAIL(f, LSQAMD_ECAPACITY, "get_grad: need %lld", (long long)f->P);
  if ((int64_t)f->hg.size() != f->P) FAIL(f, LSQAMD_EINVAL, "get_grad: no fit has run");
  if (const int rcm = refresh_mirrors(f)) return rcm;
  std::memcpy(out, f->hg.data(), sizeof(double) * f->P);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

// Data part of f / J in the reference's order (_utilities.pyx:85-93): all 1x1 rows first,
// then each block's kept modes.  Prior rows are appended by the host layer, which owns the
// prior's whitening (any W with W^T W = precision is equivalent: SURVEY.md App. B).
int lsqamd_get_f(lsqamd_fit *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "get_f: no fit has run");
  int64_t nfd = f->N;
  for (size_t b = 0; b < f->h_size.size(); ++b) nfd -= f->h_size[b] - f->h_modes[b];
  if (cap < (size_t)nfd) FAIL(f, LSQAMD_ECAPACITY, "get_f: need %lld", (long long)nfd);
  std::vector<double> r((size_t)(f->N > 0 ? f->N : 1));
  if (const int rcj = ensure_J(f)) return rcj;
  // the residual at the CURRENT point is column P of J
  HIPCHK(f, launch_copy_strided(f->st, f->J + f->P, f->ld, f->r, 1, f->N, 1));
  HIPCHK(f, hipMemcpyAsync(r.data(), f->r, sizeof(double) * f->N, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  std::vector<uint8_t> inb((size_t)(f->N > 0 ? f->N : 1), 0);
  for (size_t b = 0; b < f->h_size.size(); ++b)
    for (int64_t i = 0; i < f->h_size[b]; ++i) inb[(size_t)(f->h_row0[b] + i)] = 1;
  size_t o = 0;
  for (int64_t i = 0; i < f->N; ++i)
    if (!inb[(size_t)i]) out[o++] = r[(size_t)i];
  for (size_t b = 0; b < f->h_size.size(); ++b)
    for (int64_t m = 0; m < f->h_modes[b]; ++m) out[o++] = r[(size_t)(f->h_row0[b] + m)];
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_get_J(lsqamd_fit *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "get_J: no fit has run");
  const int64_t P = f->P;
  if (const int rcj = ensure_J(f)) return rcj;
  int64_t nfd = f->N;
  for (size_t b = 0; b < f->h_size.size(); ++b) nfd -= f->h_size[b] - f->h_modes[b];
  if (cap < (size_t)(nfd * P)) FAIL(f, LSQAMD_ECAPACITY, "get_J: need %lld", (long long)(nfd * P));
  std::vector<uint8_t> inb((size_t)(f->N > 0 ? f->N : 1), 0);
  for (size_t b = 0; b < f->h_size.size(); ++b)
    for (int64_t i = 0; i < f->h_size[b]; ++i) inb[(size_t)(f->h_row0[b] + i)] = 1;
  // copy row by row ranges with 2D copies (ld -> P)
  auto copy_rows = [&](int64_t src_row, int64_t nrows, size_t dst_row) -> hipError_t {
    return hipMemcpy2DAsync(out + dst_row * P, sizeof(double) * P, f->J + src_row * f->ld,
                            sizeof(double) * f->ld, sizeof(double) * P, (size_t)nrows,
                            hipMemcpyDeviceToHost, f->st);
  };
  size_t o = 0;
  int64_t i = 0;
  while (i < f->N) {
    if (inb[(size_t)i]) { ++i; continue; }
    int64_t j = i;
    while (j < f->N && !inb[(size_t)j]) ++j;
    HIPCHK(f, copy_rows(i, j - i, o));
    o += (size_t)(j - i);
    i = j;
  }
  for (size_t b = 0; b < f->h_size.size(); ++b) {
    if (f->h_modes[b] > 0) HIPCHK(f, copy_rows(f->h_row0[b], f->h_modes[b], o));
    o += (size_t)f->h_modes[b];
  }
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_get_jtj(lsqamd_fit *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "get_jtj: no fit has run");
  const int64_t P = f->P;
  if (cap < (size_t)(P * P)) FAIL(f, LSQAMD_ECAPACITY, "get_jtj: need %lld", (long long)(P * P));
  HIPCHK(f, launch_unpack_sym(f->st, f->redbuf, P, f->Wl, f->ldm));
  HIPCHK(f, hipMemcpy2DAsync(out, sizeof(double) * P, f->Wl, sizeof(double) * f->ldm, sizeof(double) * P,
                             (size_t)P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_get_cov(lsqamd_fit *f, double *out, size_t cap) try {
  if (!f || !out) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "get_cov: no fit has run");
  const int64_t P = f->P;
  if (cap < (size_t)(P * P)) FAIL(f, LSQAMD_ECAPACITY, "get_cov: need %lld", (long long)(P * P));
  if (!f->have_cov) {
    if (f->cov_unavailable) FAIL(f, LSQAMD_ENOTPD, "get_cov: the loss-scaled Jacobian of this robust fit had no covariance (summary.cov_status)");
    const int rc = do_covariance(f);
    if (rc < 0 && rc != LSQAMD_ENOTPD) return rc;
  }
  if (f->cov_host_valid) {       // the one-launch fit kernel mirrored it into pinned memory: no copy, no synchronisation
    std::memcpy(out, f->fit_rec.data() + lsqamd_jit::fit_host_cov((int)P), sizeof(double) * (size_t)(P * P));
    return 0;
  }
  HIPCHK(f, hipMemcpy2DAsync(out, sizeof(double) * P, f->cov, sizeof(double) * f->ldm, sizeof(double) * P,
                             (size_t)P, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

namespace {
struct DpdyPlan {
  int64_t ldv, ldn;
  double *gt, *V, *Jt, *T, *out, *wn;
  size_t bytes;
};
DpdyPlan dpdy_plan(const lsqamd_fit *f, int64_t m, void *base) {
  DpdyPlan d;
  d.ldv = rup(m, 16);
  d.ldn = rup(f->N > 0 ? f->N : 1, 16);
  Carver cv(base, 0, base == nullptr);
  d.gt = cv.take<double>(f->P * d.ldv);
  d.V = cv.take<double>(f->P * d.ldv);
  d.Jt = cv.take<double>(f->P * d.ldn);
  d.T = cv.take<double>(f->N * d.ldv);
  d.out = cv.take<double>((f->N + f->P) * d.ldv);
  d.wn = cv.take<double>(f->cfg.sum_block_sq);
  d.bytes = cv.off;
  return d;
}
}  // namespace

size_t lsqamd_dpdy_work_bytes(const lsqamd_fit *f, int64_t m) try {
  if (!f || m < 1) return 0;
  return dpdy_plan(f, m, nullptr).bytes + 256;
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_dpdy(lsqamd_fit *f, const double *gt, int64_t m, void *dev_scratch, size_t scratch_bytes,
                double *out_t, size_t cap) try {
  if (!f || !out_t || !dev_scratch) return LSQAMD_EINVAL;
  if (!f->initialised) FAIL(f, LSQAMD_EINVAL, "dpdy: no fit has run");
  const int64_t P = f->P, N = f->N;
  if (m < 1 || (!gt && m != P)) FAIL(f, LSQAMD_EINVAL, "dpdy: gt == NULL needs m == P");
  if (const int rcj = ensure_J(f)) return rcj;
  const int64_t nrows = N + (f->cfg.has_prior ? P : 0);
  if (cap < (size_t)(nrows * m)) FAIL(f, LSQAMD_ECAPACITY, "dpdy: need %lld", (long long)(nrows * m));
  char *base = (char *)dev_scratch;
  const size_t pad = (size_t)((-(intptr_t)base) & 255);
  DpdyPlan d = dpdy_plan(f, m, base + pad);
  if (scratch_bytes < d.bytes + pad) FAIL(f, LSQAMD_ENOMEM, "dpdy: scratch needs %zu bytes", d.bytes + 256);
  if (!f->have_cov) {
    const int rc = do_covariance(f);
    if (rc) return rc;
  }
  Scope sc(f, LSQAMD_T_COVAR);
  // V = cov . gt  (P x m); identity: V is cov itself
  const double *V = f->cov;
  int64_t ldv = f->ldm;
  if (gt) {
    HIPCHK(f, hipMemcpy2DAsync(d.gt, sizeof(double) * d.ldv, gt, sizeof(double) * m, sizeof(double) * m,
                               (size_t)P, hipMemcpyHostToDevice, f->st));
    GemmTN g;
    g.X = f->cov; g.ldx = f->ldm; g.Y = d.gt; g.ldy = d.ldv; g.C = d.V; g.ldc = d.ldv;
    g.M = P; g.N = m; g.K = P;
    HIPCHK(f, launch_gemm_tn(f->st, g));
    V = d.V;
    ldv = d.ldv;
  }
  const bool blocks = f->cfg.n_blocks > 0;
  if (N > 0) {
    // Jt[b][n] = w_n J[n][b]: 1x1 rows get their second factor 1/sigma here, block rows wait
    // for W^T below
    HIPCHK(f, launch_transpose_scale(f->st, f->J, f->ld, d.Jt, d.ldn, N, P, f->wdiag,
                                     blocks ? f->in_block : nullptr, 1, 0, 0));
    GemmTN g;  // T[n][o] = sum_b Jt[b][n] V[b][o]
    g.X = d.Jt; g.ldx = d.ldn; g.Y = V; g.ldy = ldv;
    g.C = blocks ? d.T : d.out; g.ldc = d.ldv;
    g.M = N; g.N = m; g.K = P;
    HIPCHK(f, launch_gemm_tn(f->st, g));
    if (blocks) {
      HIPCHK(f, launch_rows_scale_copy(f->st, d.T, d.ldv, d.out, d.ldv, N, m, nullptr, f->in_block));
      // out_b[i][o] = sum_j W_b[j][i] T_b[j][o]: the X operand is W_b itself = (stored Wt_b)^T
      for (size_t b = 0; b < f->h_size.size(); ++b) {
        const int64_t B = f->h_size[b];
        if (f->uniform_blocks && b > 0) break;
        const int64_t nb = f->uniform_blocks ? (int64_t)f->h_size.size() : 1;
        HIPCHK(f, launch_transpose_scale(f->st, f->wt + f->h_woff[b], B, d.wn + f->h_woff[b], B, B, B,
                                         nullptr, nullptr, nb, B * B, B * B));
        GemmTN w;
        w.X = d.wn + f->h_woff[b]; w.ldx = B; w.sx = B * B;
        w.Y = d.T + f->h_row0[b] * d.ldv; w.ldy = d.ldv; w.sy = B * d.ldv;
        w.C = d.out + f->h_row0[b] * d.ldv; w.ldc = d.ldv; w.sc = B * d.ldv;
        w.M = B; w.N = m; w.K = B;
        w.batch = (int32_t)nb;
        HIPCHK(f, launch_gemm_tn(f->st, w));
      }
    }
  }
  if (f->cfg.has_prior) {  // prior entries: Lambda . V
    double *op = d.out + N * d.ldv;
    if (f->cfg.prior_dense) {
      GemmTN g;
      g.X = f->prior_prec; g.ldx = P; g.Y = V; g.ldy = ldv; g.C = op; g.ldc = d.ldv;
      g.M = P; g.N = m; g.K = P;
      HIPCHK(f, launch_gemm_tn(f->st, g));
    } else {
      HIPCHK(f, launch_rows_scale_copy(f->st, V, ldv, op, d.ldv, P, m, f->prior_prec, nullptr));
    }
  }
  HIPCHK(f, hipMemcpy2DAsync(out_t, sizeof(double) * m, d.out, sizeof(double) * d.ldv, sizeof(double) * m,
                             (size_t)nrows, hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

namespace {
struct Chi2Plan {
  int64_t ldt;
  double *p, *r, *r_raw, *Dt, *T, *out;
  size_t bytes;
};
Chi2Plan chi2_plan(const lsqamd_fit *f, int64_t mc, void *base) {
  Chi2Plan d;
  d.ldt = rup(mc, 16);
  Carver cv(base, 0, base == nullptr);
  d.p = cv.take<double>(mc * f->P);
  d.r = cv.take<double>(mc * f->N);
  d.r_raw = cv.take<double>(f->cfg.n_blocks > 0 ? mc * f->N : 1);
  const bool dense = f->cfg.has_prior && f->cfg.prior_dense;
  d.Dt = cv.take<double>(dense ? f->P * d.ldt : 1);
  d.T = cv.take<double>(dense ? f->P * d.ldt : 1);
  d.out = cv.take<double>(mc);
  d.bytes = cv.off;
  return d;
}
}  // namespace

size_t lsqamd_chi2_points_work_bytes(const lsqamd_fit *f, int64_t m) try {
  if (!f || m < 1) return 0;
  return chi2_plan(f, m, nullptr).bytes + 256;
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_chi2_points(lsqamd_fit *f, const double *p, int64_t m, void *dev_scratch, size_t scratch_bytes,
                       double *chi2_out) try {
  if (!f || !p || !chi2_out || !dev_scratch || m < 0) return LSQAMD_EINVAL;
  int rc = ready(f);
  if (rc) return rc;
  if (m == 0) return 0;
  char *base = (char *)dev_scratch;
  const size_t pad = (size_t)((-(intptr_t)base) & 255);
  if (scratch_bytes <= pad) FAIL(f, LSQAMD_ENOMEM, "chi2_points: scratch too small");
  // largest chunk that fits the scratch
  int64_t mc = m;
  while (mc > 1 && chi2_plan(f, mc, nullptr).bytes + pad > scratch_bytes) mc = (mc + 1) / 2;
  if (chi2_plan(f, mc, nullptr).bytes + pad > scratch_bytes)
    FAIL(f, LSQAMD_ENOMEM, "chi2_points: scratch needs at least %zu bytes", chi2_plan(f, 1, nullptr).bytes + 256);
  if (mc > 65535) mc = 65535;  // grid.y of the model kernels
  const int64_t N = f->N, P = f->P;
  Scope sc(f, LSQAMD_T_RESIDUAL);
  for (int64_t m0 = 0; m0 < m; m0 += mc) {
    const int64_t mm = m - m0 < mc ? m - m0 : mc;
    Chi2Plan d = chi2_plan(f, mc, base + pad);
    HIPCHK(f, hipMemcpyAsync(d.p, p + m0 * P, sizeof(double) * mm * P, hipMemcpyHostToDevice, f->st));
    if (N > 0) {
      ModelArgs ma = model_args(f, d.p);
      ma.n_batch = (int32_t)mm; ma.p_stride = P; ma.out_stride = N;
      HIPCHK(f, launch_residual_ex(f->st, ma, d.r, d.r_raw));
      if (f->have_param_rows)   // prior entries whitened together with the data: rows whose "model" is a parameter
        HIPCHK(f, launch_param_rows(f->st, f->row_param, N, P, 1, d.p, f->ymean, f->wdiag,
                                    f->cfg.n_blocks > 0 ? f->in_block : nullptr, d.r, d.r_raw, 0, (int32_t)mm, P, N));
      if (f->cfg.n_blocks > 0)
        HIPCHK(f, launch_block_whiten_vec(f->st, f->wt, f->blk_row0, f->blk_size, f->blk_woff,
                                          f->cfg.n_blocks, f->cfg.max_block, d.r_raw, d.r, (int32_t)mm, N,
                                          nullptr));
      HIPCHK(f, launch_rows_sumsq(f->st, d.r, N, N, mm, d.out, 0));
    } else {
      HIPCHK(f, hipMemsetAsync(d.out, 0, sizeof(double) * mm, f->st));
    }
    if (f->cfg.has_prior && f->adds_prior)
      HIPCHK(f, launch_prior_chi2_points(f->st, P, f->prior_prec, f->cfg.prior_dense, f->prior_mean, d.p, mm,
                                         d.Dt, d.T, d.ldt, d.out));
    rc = do_reduce(f, d.out, mm);
    if (rc) return rc;
    HIPCHK(f, hipMemcpyAsync(chi2_out + m0, d.out, sizeof(double) * mm, hipMemcpyDeviceToHost, f->st));
    HIPCHK(f, hipStreamSynchronize(f->st));
    f->nfev += (int32_t)mm;
  }
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_handoff_stats(int64_t *out3) try {
  if (!out3) return LSQAMD_EINVAL;
  for (int i = 0; i < 3; ++i) out3[i] = g_handoff[i].load();
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

void lsqamd_debug_set_potf2_stamps(void *dev_ptr) { lsqamd::g_potf2_dbg = (long long *)dev_ptr; }

// self-tests of the boundary's own machinery, runnable without a GPU (tests/test_abi.py)
int lsqamd_debug_throw(lsqamd_fit *f, int32_t kind) try {
  if (kind == 1) throw std::bad_alloc();
  if (kind == 2) throw std::runtime_error("lsqamd_debug_throw");
  if (kind == 3) throw 42;
  if (kind == 4) { std::vector<double> v; v.reserve(v.max_size()); }   // a real allocation failure (std::length_error / bad_alloc)
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

// The runtime behaviour capture_reset (common.h) exists for, reproduced deterministically: a ThreadLocal capture on `stream`,
// ONE legacy-stream hipMemcpy from another thread while it is open, then the recovery.  report[0] = what the intruder's
// hipMemcpy returned, [1] = what hipStreamEndCapture returned, [2] = the stream's capture status after EndCapture
// (2 = still "invalidated": the runtime defect), [3] = the status after capture_reset (0 = usable), [4] = result of an
// eager copy + synchronise on the stream afterwards (0 = success), [5] = the value that copy delivered (42).
int lsqamd_debug_capture_selftest(void *stream, int32_t *report) try {
  if (!report) return LSQAMD_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!st) return LSQAMD_EINVAL;
  for (int i = 0; i < 6; ++i) report[i] = -1;
  int32_t *dev = nullptr, *dev2 = nullptr;
  if (hipMalloc(&dev, 64) != hipSuccess || hipMalloc(&dev2, 64) != hipSuccess) return LSQAMD_EHIP;
  const int32_t v42 = 42;
  (void)hipMemcpyAsync(dev, &v42, sizeof v42, hipMemcpyHostToDevice, st);
  (void)hipStreamSynchronize(st);
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return LSQAMD_EHIP; }
  (void)hipMemcpyAsync(dev2, dev, 4, hipMemcpyDeviceToDevice, st);
  {
    std::atomic<int> rc{-1};
    std::thread other([&] {
      int32_t h = 0;
      rc.store((int)hipMemcpy(&h, dev, 4, hipMemcpyDeviceToHost));   // legacy default stream, from ANOTHER thread
      (void)hipGetLastError();
    });
    other.join();
    report[0] = rc.load();
  }
  (void)hipMemcpyAsync(dev2, dev, 4, hipMemcpyDeviceToDevice, st);
  (void)hipGetLastError();
  hipGraph_t g = nullptr;
  report[1] = (int32_t)hipStreamEndCapture(st, &g);
  (void)hipGetLastError();
  if (g) (void)hipGraphDestroy(g);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cs);
  report[2] = (int32_t)cs;
  lsqamd::capture_reset(st);
  (void)hipStreamIsCapturing(st, &cs);
  report[3] = (int32_t)cs;
  int32_t back = 0;
  hipError_t e = hipMemcpyAsync(&back, dev, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  report[4] = (int32_t)e;
  report[5] = back;
  (void)hipGetLastError();
  (void)hipFree(dev);
  (void)hipFree(dev2);
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

// the work lists of the J^T J launch (host arithmetic only): G == 0: the plain list; G >= 1: the list of the grouped exchange
// in group-major order inside every XCD run (rows[G + 1] = tile-row bounds, count[G] = entries per group).  -> entries
int64_t lsqamd_debug_syrk_work(int64_t P, int32_t splits, int32_t G, const int32_t *rows, int32_t *out4, int32_t *count) try {
  if (P < 1 || splits < 1 || !out4) return -1;
  if (G <= 0) {
    syrk_work_fill(P, splits, out4);
    return syrk_work_count(P, splits);
  }
  if (!rows || !count || G > 8) return -1;
  syrk_work_fill_grouped(P, splits, G, rows, out4, count);
  return syrk_work_count(P, splits);
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_debug_per_device_once(int32_t dev, int32_t reset) try {
  // how often has the "set the kernel attributes" action of a PerDeviceOnce run for device `dev`?  (the bookkeeping that
  // guards every kernel-attribute call of the library, on an instance of its own: no HIP call)
  static lsqamd::PerDeviceOnce once;
  static std::atomic<int> runs[lsqamd::PerDeviceOnce::kMaxDev + 1];
  if (reset) {
    once.done.store(0);
    for (auto &r : runs) r.store(0);
    return 0;
  }
  const int slot = (dev >= 0 && dev < lsqamd::PerDeviceOnce::kMaxDev) ? dev : lsqamd::PerDeviceOnce::kMaxDev;
  const hipError_t e = once.run_for(dev, [slot] { runs[slot].fetch_add(1); return hipSuccess; });
  if (e != hipSuccess) return LSQAMD_EHIP;
  return runs[slot].load();
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(nullptr);)

// introspection for tests: bit0 uniform-block batched whitening, bits 8.. split-K factor
int64_t lsqamd_debug_flags(const lsqamd_fit *f) try {
  if (!f) return -1;
  return (int64_t)(f->uniform_blocks ? 1 : 0) | (int64_t)(f->used_synth ? 2 : 0) | (int64_t)(f->graph_launches > 0 ? 4 : 0) |
         (int64_t)(f->used_nrm ? 16 : 0) | (int64_t)(f->used_one_launch ? 32 : 0) |
         (int64_t)(f->jit || (!f->progs.empty() && f->progs_compiled == (int)f->progs.size()) ? 8 : 0) |
         ((int64_t)f->splits << 8) |
         ((int64_t)f->h_size.size() << 32);
} LSQAMD_ABI_CATCH((void)lsqamd::abi_exception(nullptr); return 0;)

int lsqamd_timing_enable(lsqamd_fit *f, int32_t on) try {
  if (!f) return LSQAMD_EINVAL;
  f->timing = on != 0;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_timing_get(lsqamd_fit *f, int32_t which, double *total_ms, int64_t *count) try {
  if (!f || which < 0 || which >= LSQAMD_T_COUNT) return LSQAMD_EINVAL;
  resolve_timers(f);
  if (total_ms) *total_ms = f->timers[which].total_ms;
  if (count) *count = f->timers[which].count;
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

int lsqamd_timing_reset(lsqamd_fit *f) try {
  if (!f) return LSQAMD_EINVAL;
  resolve_timers(f);
  for (auto &t : f->timers) { t.total_ms = 0.0; t.count = 0; }
  return 0;
} LSQAMD_ABI_CATCH(return lsqamd::abi_exception(f);)

}  // extern "C"
