// lfa_stage.cpp — host buffers under the write table's ops
// (lfa_atomic_write_staged, lfa_zero_copy_addr): the staging slots, the
// zero-copy classification of an operand and the temporary registrations of
// pageable memory.
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stdlib.h>

#include "lfa_capi_int.h"
#include "lfa_signal.h"

namespace {
// Staging contexts for lfa_atomic_write_staged: two streams, the slot events
// and an HBM staging buffer that only grows.  kStageSlots per device, each
// with its own lock, so concurrent host-buffer callers on one device run at
// once instead of queueing behind one caller's PCIe transfer;
// a caller takes a free slot, and waits on one only when all are busy.
// Created on first use and kept for the life of the process (a hipMalloc +
// hipFree per call costs milliseconds and serialises the device).
struct StagingCtx {
  pthread_mutex_t lock = PTHREAD_MUTEX_INITIALIZER;
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t in_done[2] = {}, out_done[2] = {};
  char *dev = nullptr;
  size_t cap = 0;
};
constexpr int kStageSlots = 4;
StagingCtx g_staging[kMaxDevices][kStageSlots];
unsigned g_stage_next[kMaxDevices];

// A staging slot of device `devno`, locked; staging_release unlocks it.
StagingCtx &staging_lock(int devno) {
  for (StagingCtx &c : g_staging[devno])
    if (!pthread_mutex_trylock(&c.lock)) return c;
  StagingCtx &c = g_staging[devno][__atomic_fetch_add(&g_stage_next[devno], 1u,
                                                      __ATOMIC_RELAXED) % kStageSlots];
  pthread_mutex_lock(&c.lock);
  return c;
}

int staging_acquire(StagingCtx &c, size_t bytes) {
  if (!c.s_in) {
    if (hipStreamCreateWithFlags(&c.s_in, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c.s_out, hipStreamNonBlocking) != hipSuccess)
      return -LFA_ENOMEM;
    for (int i = 0; i < 2; i++)
      if (hipEventCreateWithFlags(&c.in_done[i], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&c.out_done[i], hipEventDisableTiming) != hipSuccess)
        return -LFA_ENOMEM;
  }
  if (c.cap < bytes) {
    if (c.dev) hipFree(c.dev);
    c.dev = nullptr;
    c.cap = 0;
    if (hipMalloc((void **)&c.dev, bytes) != hipSuccess) return -LFA_ENOMEM;
    c.cap = bytes;
  }
  return 0;
}

bool zero_copy_on() {
  const char *e = lfa_param("LFA_HOST_ZERO_COPY");
  return !e || strtol(e, nullptr, 0);
}

// Temporary registrations: pageable operands lfa_atomic_write_staged pins
// for one call (hipHostRegister), refcounted by exact (address, length) so
// callers combining the same buffer share one.  A registration's page range
// is in this table from before hipHostRegister until after hipHostUnregister
// (states PENDING -> READY -> DYING), and every classification checks the
// table first: a page range in it is never handed out as a zero-copy address
// (the call that made it may unregister it at any moment), and an operand
// overlapping another call's registration is staged.  g_reg_lock covers the
// table and the classifications — never a registration, a kernel or a
// stream synchronisation (holding it across the
// combine stalled every endpoint's submit for the whole PCIe transfer).
enum { kRegFree = 0, kRegPending, kRegReady, kRegDying };
struct TempReg {
  int state;
  uintptr_t lo, hi;  // the page range
  const void *p;
  size_t bytes;
  void *d;           // its device address once READY
  int refs;
};
constexpr int kTempRegs = 64;
TempReg g_temp[kTempRegs];
pthread_mutex_t g_reg_lock = PTHREAD_MUTEX_INITIALIZER;
constexpr uintptr_t kPage = 4096;

// The entry overlapping the pages of [p, p + bytes), or -1 (g_reg_lock held).
int temp_find(const void *p, size_t bytes) {
  const uintptr_t lo = (uintptr_t)p & ~(kPage - 1);
  const uintptr_t hi = ((uintptr_t)p + (bytes ? bytes : 1) + kPage - 1) & ~(kPage - 1);
  for (int i = 0; i < kTempRegs; i++)
    if (g_temp[i].state != kRegFree && g_temp[i].lo < hi && lo < g_temp[i].hi) return i;
  return -1;
}

// The address a kernel on device `devno` uses for operand p, or null when
// the operand must be staged: device memory of this device as it is, pinned
// or registered host memory through its device mapping (zero-copy: the
// combine reads and writes it over PCIe) — never a temporary registration.
// *pageable: p is host memory HIP does not know, which the caller may
// register for the call.  g_reg_lock held.
void *zero_copy_addr(const void *p, size_t bytes, int devno, bool *pageable) {
  hipPointerAttribute_t a;
  *pageable = false;
  if (temp_find(p, bytes) >= 0) return nullptr;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    *pageable = true;
    return nullptr;
  }
  if (a.type == hipMemoryTypeUnregistered) *pageable = true;
  if (a.type == hipMemoryTypeHost) return a.devicePointer;
  if (a.type == hipMemoryTypeDevice && a.device == devno) return const_cast<void *>(p);
  return nullptr;
}

// Pin pageable operand p (bytes long) for one call; its device address, or
// null if the runtime refuses (overlapping registrations, read-only pages):
// the caller then stages.
void *register_for_call(const void *p, size_t bytes) {
  void *d = nullptr;
  if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterMapped) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (hipHostGetDevicePointer(&d, const_cast<void *>(p), 0) != hipSuccess || !d) {
    (void)hipGetLastError();
    hipHostUnregister(const_cast<void *>(p));
    return nullptr;
  }
  return d;
}

// A temporary registration of exactly [p, p + bytes) for this call: a READY
// one shared (refs + 1), else a new one; its index and device address, or -1
// (the pages overlap another call's registration, another call holds one —
// `mine`, this call's other operand's, aside — or the runtime refused): the
// caller stages.
int temp_take(const void *p, size_t bytes, void **d, int mine) {
  pthread_mutex_lock(&g_reg_lock);
  int i = temp_find(p, bytes);
  if (i >= 0) {
    TempReg &t = g_temp[i];
    const bool share = t.state == kRegReady && t.p == p && t.bytes == bytes;
    if (share) {
      t.refs++;
      *d = t.d;
    }
    pthread_mutex_unlock(&g_reg_lock);
    return share ? i : -1;
  }
  // one call registers at a time: hipHostRegister / hipHostUnregister from
  // several threads at once slow each other down (4 threads of pageable
  // 2 MiB combines: 29x one call, against 3.7x when they stage;
  // profiles/r06_threads_probe_before.jsonl), so while another call holds or makes
  // a registration this one takes the staged pipeline, which overlaps
  int busy = 0;
  for (int k = 0; k < kTempRegs; k++) busy += k != mine && g_temp[k].state != kRegFree;
  for (i = 0; i < kTempRegs && g_temp[i].state != kRegFree; i++) {
  }
  if (busy || i == kTempRegs) {
    pthread_mutex_unlock(&g_reg_lock);
    return -1;
  }
  g_temp[i] = TempReg{kRegPending, (uintptr_t)p & ~(kPage - 1),
                      ((uintptr_t)p + bytes + kPage - 1) & ~(kPage - 1), p, bytes, nullptr, 1};
  pthread_mutex_unlock(&g_reg_lock);
  void *dp = register_for_call(p, bytes);  // outside the lock: milliseconds
  pthread_mutex_lock(&g_reg_lock);
  if (dp) {
    g_temp[i].state = kRegReady;
    g_temp[i].d = dp;
  } else {
    g_temp[i].state = kRegFree;
  }
  pthread_mutex_unlock(&g_reg_lock);
  *d = dp;
  return dp ? i : -1;
}

// Calls in the staged pipeline right now: a call does not register its
// pageable operands while any is (lfa_atomic_write_staged).
int g_staged_calls;

// Pageable buckets below this stage instead of registering for the call
// (LFA_HOST_REGISTER_BYTES, default 64 MiB): below it the gain is a few
// hundred microseconds, and a registration stalls concurrent callers.
size_t register_min_bytes() {
  // read per call (a call this size costs milliseconds): tests move it
  const char *e = lfa_param("LFA_HOST_REGISTER_BYTES");
  return e ? (size_t)strtoull(e, nullptr, 0) : (size_t)64 << 20;
}

// This call is done with registration i: the last user unregisters it (the
// pages stay in the table as DYING until hipHostUnregister has returned).
void temp_drop(int i) {
  if (i < 0) return;
  pthread_mutex_lock(&g_reg_lock);
  const bool last = --g_temp[i].refs == 0;
  if (last) g_temp[i].state = kRegDying;
  const void *p = g_temp[i].p;
  pthread_mutex_unlock(&g_reg_lock);
  if (!last) return;
  hipHostUnregister(const_cast<void *>(p));
  pthread_mutex_lock(&g_reg_lock);
  g_temp[i].state = kRegFree;
  pthread_mutex_unlock(&g_reg_lock);
}
}  // namespace

extern "C" {

int lfa_atomic_write_staged(enum lfa_op op, enum lfa_datatype dt, void *dst,
                            const void *src, size_t cnt, size_t chunk_bytes) {
  if ((unsigned)op >= LFA_WRITE_OP_CNT || !reducible(op, dt))
    return -LFA_EOPNOTSUPP;
  if (cnt && (!dst || !src)) return -LFA_EINVAL;
  if (!cnt) return 0;
  const size_t esz = lfa_reduce_datatype_size(dt);
  if (!chunk_bytes) chunk_bytes = 32u << 20;
  size_t per = chunk_bytes / esz;
  if (!per) per = 1;
  if (per > cnt) per = cnt;
  // chunk slots keep 256-byte alignment so the vector body applies
  const size_t slot = (per * esz + 255) & ~(size_t)255;
  int devno = 0;
  if (hipGetDevice(&devno) != hipSuccess || devno < 0 || devno >= kMaxDevices)
    return -LFA_EINVAL;
  const size_t bytes = cnt * esz;
  bool pd = false, ps = false;
  void *zd = nullptr, *zs = nullptr;
  int reg[2] = {-1, -1};
  if (zero_copy_on()) {
    pthread_mutex_lock(&g_reg_lock);
    zd = zero_copy_addr(dst, bytes, devno, &pd);
    zs = zero_copy_addr(src, bytes, devno, &ps);
    pthread_mutex_unlock(&g_reg_lock);
    if ((zd || pd) && (zs || ps) && (pd || ps) && bytes >= register_min_bytes() &&
        !__atomic_load_n(&g_staged_calls, __ATOMIC_RELAXED)) {
      // large pageable operands of a call that is alone are pinned for the
      // call: registration + the zero-copy combine beats the runtime's
      // staging of pageable memory (256 MiB 15.4 -> 11.5 ms,
      // profiles/r05_zero_copy_pageable.log).  Not below
      // LFA_HOST_REGISTER_BYTES, and not while another call is staging:
      // registering and unregistering stall every other caller's copies and
      // kernels (4 threads of 2 MiB: 29x one call registering, 3.7x
      // staging; profiles/r06_threads_probe_*.jsonl)
      if (pd) reg[0] = temp_take(dst, bytes, &zd, -1);
      if (ps && src == dst) zs = zd;
      else if (ps) reg[1] = temp_take(src, bytes, &zs, reg[0]);
    }
    if (!zd || !zs) {
      // stage instead
      zd = zs = nullptr;
      for (int &i : reg) temp_drop(i), i = -1;
    }
  }
  const bool staged = !(zd && zs);
  if (staged) __atomic_add_fetch(&g_staged_calls, 1, __ATOMIC_RELAXED);
  StagingCtx &c = staging_lock(devno);
  if (zd && zs) {
    // every operand reachable from the device: one combine over the mapped
    // buffers, no HBM round trip (256 MiB float SUM, both pinned: 9.96 ms
    // against 11.22 ms staged, profiles/r05_zero_copy.log)
    int ret = staging_acquire(c, 0);
    if (!ret) ret = kOps[op]->write(dt | LFA_WRITE_MAPPED, zd, zs, cnt, c.s_out, 0);
    if (hipStreamSynchronize(c.s_out) != hipSuccess && !ret) ret = -LFA_EIO;
    pthread_mutex_unlock(&c.lock);
    for (int i : reg) temp_drop(i);
    return ret;
  }
  int ret = staging_acquire(c, 4 * slot);
  if (!ret) {
    for (int i = 0; i < 2; i++) hipEventRecord(c.out_done[i], c.s_out);
    for (size_t off = 0, k = 0; off < cnt && !ret; off += per, k ^= 1) {
      const size_t n = cnt - off < per ? cnt - off : per;
      char *dd = c.dev + k * 2 * slot, *ds = dd + slot;
      // slot reuse: the D2H of the chunk two back must have drained it
      hipStreamWaitEvent(c.s_in, c.out_done[k], 0);
      hipMemcpyAsync(dd, (char *)dst + off * esz, n * esz, hipMemcpyDefault, c.s_in);
      hipMemcpyAsync(ds, (const char *)src + off * esz, n * esz, hipMemcpyDefault,
                     c.s_in);
      hipEventRecord(c.in_done[k], c.s_in);
      hipStreamWaitEvent(c.s_out, c.in_done[k], 0);
      ret = kOps[op]->write(dt, dd, ds, n, c.s_out, 0);
      hipMemcpyAsync((char *)dst + off * esz, dd, n * esz, hipMemcpyDefault, c.s_out);
      hipEventRecord(c.out_done[k], c.s_out);
    }
    if (hipStreamSynchronize(c.s_out) != hipSuccess && !ret) ret = -LFA_EIO;
    if (hipStreamSynchronize(c.s_in) != hipSuccess && !ret) ret = -LFA_EIO;
  }
  pthread_mutex_unlock(&c.lock);
  if (staged) __atomic_sub_fetch(&g_staged_calls, 1, __ATOMIC_RELAXED);
  return ret;
}

void *lfa_zero_copy_addr(const void *p, int device) {
  if (!p || !zero_copy_on()) return nullptr;
  bool pageable;
  pthread_mutex_lock(&g_reg_lock);
  void *r = zero_copy_addr(p, 1, device, &pageable);
  pthread_mutex_unlock(&g_reg_lock);
  return r;
}

int lfa__temp_registrations(void) {
  int n = 0;
  pthread_mutex_lock(&g_reg_lock);
  for (const TempReg &t : g_temp) n += t.state != kRegFree;
  pthread_mutex_unlock(&g_reg_lock);
  return n;
}

}  // extern "C"
