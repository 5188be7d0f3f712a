// What a handle takes from the runtime besides its workspace, recycled over the process (host code only, gfx950 build):
// pinned blocks, events and streams -- creating and releasing one costs tens to hundreds of microseconds, more than a small
// fit (declared in fit_state.h; batch.hip shares the events and streams).  Also the process-wide things that ride on them:
// the counters of the polled pinned-memory hand-offs, the poison of the LSQAMD_POISON_PINNED test knob, and the per-handle
// event timers (take_event, resolve_timers) whose events come from here.
#include <cstdint>
#include <cstdlib>
#include <atomic>
#include <map>
#include <mutex>
#include <utility>

#include "host.h"

namespace lsqamd_host {

// ---- process-wide recycling of pinned blocks and events (see fit_state.h) -------------------------------------------
int current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = -1; }
  return d;
}

namespace {
struct Recycler {
  std::mutex mu;
  std::multimap<std::pair<int, size_t>, void *> pinned;   // (device, size class) -> block
  size_t pinned_bytes = 0;
  std::multimap<int, hipEvent_t> events;
  std::multimap<int, hipStream_t> streams;
};
Recycler &recycler() {
  static Recycler *r = new Recycler;    // never destroyed: no runtime calls from a static destructor at exit
  return *r;
}
constexpr size_t PIN_CLASS = 4096, PIN_KEEP_MAX = 64 << 10, PIN_KEEP_TOTAL = 2 << 20;
}  // namespace

// Hand-offs through polled pinned memory (wait_record, run_one_launch), over the process: snapshots that did not verify (yet),
// hand-offs served from device memory after the stream had drained, words the test knob LSQAMD_VERIFY_HANDOFF=1 found different
// from the device's own copy (must stay 0).  lsqamd_handoff_stats reads them.
std::atomic<int64_t> g_handoff[3];

// LSQAMD_POISON_PINNED=1 (test knob): every pinned block handed out, and every region a kernel is about to publish into, is
// filled with a recognisable NaN first -- a host that acts on words the device has not written yet then acts on NaNs, loudly
bool poison_pinned() {
  static const bool on = [] { const char *e = getenv("LSQAMD_POISON_PINNED"); return e && e[0] == '1'; }();
  return on;
}
void poison_fill(void *p, size_t bytes) {
  const uint64_t nan_bits = 0x7ff8dead0000beefULL;
  uint64_t *w = static_cast<uint64_t *>(p);
  for (size_t i = 0; i < bytes / 8; ++i) w[i] = nan_bits;
}

void *pinned_take(size_t bytes, size_t *granted) {
  const size_t cls = (bytes + PIN_CLASS - 1) / PIN_CLASS * PIN_CLASS;
  *granted = cls;
  const int dev = current_device();
  {
    Recycler &r = recycler();
    std::lock_guard<std::mutex> lk(r.mu);
    auto it = r.pinned.find({dev, cls});
    if (it != r.pinned.end()) {
      void *p = it->second;
      r.pinned.erase(it);
      r.pinned_bytes -= cls;
      if (poison_pinned()) poison_fill(p, cls);
      return p;
    }
  }
  void *p = nullptr;
  if (hipHostMalloc(&p, cls, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (poison_pinned()) poison_fill(p, cls);
  return p;
}

void pinned_give(void *p, size_t granted, int dev_taken) {
  if (!p) return;
  const int dev = dev_taken >= 0 ? dev_taken : current_device();
  if (granted > 0 && granted <= PIN_KEEP_MAX && dev >= 0) {
    Recycler &r = recycler();
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.pinned_bytes + granted <= PIN_KEEP_TOTAL) {
      r.pinned.insert({{dev, granted}, p});
      r.pinned_bytes += granted;
      return;
    }
  }
  (void)hipHostFree(p);
}

hipEvent_t event_take() {
  const int dev = current_device();
  {
    Recycler &r = recycler();
    std::lock_guard<std::mutex> lk(r.mu);
    auto it = r.events.find(dev);
    if (it != r.events.end()) {
      hipEvent_t e = it->second;
      r.events.erase(it);
      return e;
    }
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void event_give(hipEvent_t e, int dev_taken) {
  if (!e) return;
  const int dev = dev_taken >= 0 ? dev_taken : current_device();
  if (dev >= 0) {
    Recycler &r = recycler();
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.events.size() < 256) {
      r.events.insert({dev, e});
      return;
    }
  }
  (void)hipEventDestroy(e);
}

hipStream_t stream_take() {
  const int dev = current_device();
  {
    Recycler &r = recycler();
    std::lock_guard<std::mutex> lk(r.mu);
    auto it = r.streams.find(dev);
    if (it != r.streams.end()) {
      hipStream_t s = it->second;
      r.streams.erase(it);
      return s;
    }
  }
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return s;
}

void stream_give(hipStream_t s, int dev_taken) {
  if (!s) return;
  const int dev = dev_taken >= 0 ? dev_taken : current_device();      // (filed under the device it was created on, whichever device the calling thread has current)
  if (dev >= 0) {
    Recycler &r = recycler();
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.streams.size() < 16) {
      r.streams.insert({dev, s});
      return;
    }
  }
  (void)hipStreamDestroy(s);
}

// ---- the handle's event timers (Scope, fit_state.h) ------------------------------------------------------------------
hipEvent_t take_event(lsqamd_fit *f) {  // events are recycled: creating one costs ~10 us
  hipEvent_t e = nullptr;
  if (!f->event_pool.empty()) {
    e = f->event_pool.back();
    f->event_pool.pop_back();
  } else {
    e = event_take();
  }
  return e;
}

// Between the steps of a fit the pairs just pile up: reading them back costs ~100 us of host time per step (18 event
// queries), all of it between the arrival of a step's record and the first launch of the next -- measured as GPU idle
// time with rocprofv3 at the 8-GPU shard shape.  They are read when somebody asks (lsqamd_get_timers / _reset /
// _finish) or when a few hundred have piled up.
void resolve_timers(lsqamd_fit *f, bool only_if_many) {
  if (only_if_many) {
    size_t n = 0;
    for (auto &t : f->timers) n += t.pending.size();
    if (n < 512) return;
  }
  for (auto &t : f->timers) {      // intervals another timer owns the events of: before those events are recycled below
    for (auto &pr : t.pending_shared) {
      (void)hipEventSynchronize(pr.second);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
        t.total_ms += ms;
        t.count += 1;
      }
    }
    t.pending_shared.clear();
  }
  for (auto &t : f->timers) {
    for (auto &pr : t.pending) {
      (void)hipEventSynchronize(pr.second);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
        t.total_ms += ms;
        t.count += 1;
      }
      f->event_pool.push_back(pr.first);
      f->event_pool.push_back(pr.second);
    }
    t.pending.clear();
  }
}

}  // namespace lsqamd_host
