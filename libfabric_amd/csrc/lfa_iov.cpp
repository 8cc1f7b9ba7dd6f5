// lfa_iov.cpp — the host side of the list (fi_ioc) forms: one launch for
// every segment of a call (lfa_atomic_writev_async, lfa_reduce_treev_async,
// lfa_atomic_readwritev_async, lfa_atomic_swapv_async).
// The table's layout: lfa_iov.h; its builder: lfa_iov_table.h.
#include <hip/hip_runtime_api.h>
#include <pthread.h>

#include "lfa_capi_int.h"
#include "lfa_iov_table.h"

extern "C" int lfa__iov_check(const struct lfa_ioc *, const struct lfa_ioc *, int, size_t,
                              size_t);
extern "C" int lfa__iov_fetch_check(const struct lfa_ioc *, const struct lfa_ioc *, int,
                                    const struct lfa_ioc *, int, const struct lfa_ioc *, size_t,
                                    size_t);

namespace {

// A table too large for the kernel arguments goes through a ring of
// kIovSlots slots per device.  A slot is a pinned host buffer the call fills
// and a device buffer hipMemcpyAsync copies it to on the caller's stream,
// just ahead of the kernel; the event recorded behind the kernel says when
// both may be reused.  Slots are taken round robin, so the one a call gets
// is the oldest: its event has almost always completed (hipEventQuery), and
// only a caller with more than kIovSlots such calls in flight waits for the
// oldest launch (hipEventSynchronize).  Slots start empty and grow to the
// largest table they have carried (a power of two from 64 KiB; at most
// 128 KiB for LFA_IOV_MAX binary segments, 256 KiB for LFA_IOV_MAX fetch or
// compare segments, 1 MiB for LFA_IOV_MAX segments of 15 inputs), so steady
// state allocates nothing.
constexpr int kIovSlots = 8;
struct IovSlot {
  uint64_t *host = nullptr, *dev = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  bool busy = false;
};
struct IovRing {
  pthread_mutex_t lock = PTHREAD_MUTEX_INITIALIZER;
  IovSlot slot[kIovSlots];
  unsigned next = 0;
};
IovRing g_iov_ring[kMaxDevices];

// The ring's next slot, idle and at least `bytes` large (ring lock held).
int iov_slot_take(IovRing &ring, size_t bytes, IovSlot **out) {
  IovSlot &s = ring.slot[ring.next++ % kIovSlots];
  if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess)
    return -LFA_EIO;
  if (s.busy) {
    hipError_t e = hipEventQuery(s.done);
    if (e == hipErrorNotReady) e = hipEventSynchronize(s.done);
    if (e != hipSuccess) return -LFA_EIO;
    s.busy = false;
  }
  if (s.cap < bytes) {
    size_t cap = (size_t)64 << 10;
    while (cap < bytes) cap *= 2;
    if (s.host) hipHostFree(s.host);
    if (s.dev) hipFree(s.dev);
    s.host = s.dev = nullptr;
    s.cap = 0;
    if (hipHostMalloc((void **)&s.host, cap, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&s.dev, cap) != hipSuccess)
      return -LFA_ENOMEM;
    s.cap = cap;
  }
  *out = &s;
  return 0;
}

// Launch `go(args, ntile)` with the table in the kernel arguments, or in a
// ring slot copied on `stream` ahead of the kernel.
template <typename Go>
int iov_launch(const IovTable &t, void *stream, Go &&go) {
  lfa_iov_args a;
  memset(&a, 0, sizeof(a));
  a.nseg = (uint32_t)t.nseg();
  a.nin = t.nin;
  a.direct = t.direct;
  const unsigned ntile = t.first.back();
  const size_t words = t.words();
  if (words <= LFA_IOV_INLINE) {
    t.write(a.inl);
    return go(&a, ntile);
  }
  int devno = 0;
  if (hipGetDevice(&devno) != hipSuccess || devno < 0 || devno >= kMaxDevices)
    return -LFA_EINVAL;
  IovRing &ring = g_iov_ring[devno];
  pthread_mutex_lock(&ring.lock);
  IovSlot *s = nullptr;
  int rc = iov_slot_take(ring, words * 8, &s);
  if (!rc) {
    t.write(s->host);
    if (hipMemcpyAsync(s->dev, s->host, words * 8, hipMemcpyHostToDevice,
                       (hipStream_t)stream) != hipSuccess)
      rc = -LFA_EIO;
  }
  if (!rc) {
    a.tab = s->dev;
    rc = go(&a, ntile);
    // the copy is enqueued: the slot stays taken until the stream passes here
    s->busy = true;
    if (hipEventRecord(s->done, (hipStream_t)stream) != hipSuccess && !rc) rc = -LFA_EIO;
  }
  pthread_mutex_unlock(&ring.lock);
  return rc;
}

thread_local IovTable t_iov;

}  // namespace

extern "C" {

int lfa_atomic_writev_async(enum lfa_op op, enum lfa_datatype dt,
                            const struct lfa_ioc *dst, const struct lfa_ioc *src,
                            size_t nseg, void *stream) {
  if ((unsigned)op >= LFA_WRITE_OP_CNT || !reducible(op, dt)) return -LFA_EOPNOTSUPP;
  if (!nseg) return 0;
  const size_t esz = lfa_reduce_datatype_size(dt);
  int rc = lfa__iov_check(dst, src, 1, nseg, esz);
  if (rc) return rc;
  IovTable &t = t_iov;
  t.reset(1);
  size_t only = 0;
  for (size_t i = 0; i < nseg; i++) {
    if (!dst[i].count) continue;
    const void *in = src[i].addr;
    if ((rc = t.add(dst[i].addr, dst[i].count, &in, esz))) return rc;
    only = i;
  }
  if (!t.nseg()) return 0;
  // One segment is what lfa_atomic_write_async takes: its kernels choose
  // their tiling and store policy by size (taper, nt stores from 192 MiB),
  // which a 256 MiB segment keeps.
  if (t.nseg() == 1)
    return kOps[op]->write(dt, dst[only].addr, src[only].addr, dst[only].count, stream, 0);
  return iov_launch(t, stream, [&](const lfa_iov_args *a, unsigned ntile) {
    return kOps[op]->writev(dt, a, ntile, stream);
  });
}

int lfa_reduce_treev_async(enum lfa_op op, enum lfa_datatype dt,
                           const struct lfa_ioc *dst, const void *const *srcs,
                           int nsrc, size_t nseg, void *stream) {
  if ((unsigned)op > LFA_BXOR || !reducible(op, dt)) return -LFA_EOPNOTSUPP;
  if (nsrc < 1 || nsrc > LFA_TREE_MAX) return -LFA_EINVAL;
  if (!nseg) return 0;
  const size_t esz = lfa_reduce_datatype_size(dt);
  int rc = lfa__iov_check(dst, nullptr, 0, nseg, esz);
  if (rc) return rc;
  if (!srcs) return -LFA_EINVAL;
  for (size_t i = 0; i < nseg; i++)
    for (int k = 0; k < nsrc && dst[i].count; k++)
      if (!srcs[i * nsrc + k]) return -LFA_EINVAL;
  if (nsrc >= 2 * LFA_IOV_TREE_LEAVES) {
    // The fused form is built for up to LFA_IOV_TREE_LEAVES leaves (the
    // fan-in of a node's GPUs; liblfa.so's size).  A wider tree
    // runs one tree launch per segment: the same bits, and with 16 or more
    // input streams per segment the launch is no longer the cost.
    for (size_t i = 0; i < nseg && !rc; i++)
      rc = lfa_reduce_tree_async(op, dt, dst[i].addr, srcs + i * nsrc, nsrc, dst[i].count,
                                 stream);
    return rc;
  }
  IovTable &t = t_iov;
  // one input is a copy, as in lfa_reduce_tree_async: the binary form's
  // ATOMIC_WRITE over bytes, a segment that is its own input left alone
  const bool copy = nsrc == 1;
  t.reset(copy ? 1 : (uint32_t)nsrc);
  size_t only = 0;
  for (size_t i = 0; i < nseg; i++) {
    if (!dst[i].count || (copy && srcs[i] == dst[i].addr)) continue;
    if ((rc = copy ? t.add(dst[i].addr, dst[i].count * esz, srcs + i, 1)
                   : t.add(dst[i].addr, dst[i].count, srcs + i * nsrc, esz)))
      return rc;
    only = i;
  }
  if (!t.nseg()) return 0;
  if (t.nseg() == 1)
    return lfa_reduce_tree_async(op, dt, dst[only].addr, srcs + only * nsrc, nsrc,
                                 dst[only].count, stream);
  return iov_launch(t, stream, [&](const lfa_iov_args *a, unsigned ntile) {
    return copy ? kOps[LFA_ATOMIC_WRITE]->writev(LFA_UINT8, a, ntile, stream)
                : kOps[op]->treev(dt, a, nsrc, ntile, stream);
  });
}

int lfa_atomic_readwritev_async(enum lfa_op op, enum lfa_datatype dt,
                                const struct lfa_ioc *dst, const struct lfa_ioc *src,
                                const struct lfa_ioc *res, size_t nseg, void *stream) {
  if ((unsigned)op >= LFA_READWRITE_OP_CNT || (unsigned)dt >= LFA_DATATYPE_CNT ||
      !in_rw_table(op, dt))
    return -LFA_EOPNOTSUPP;
  if (!nseg) return 0;
  const size_t esz = lfa_datatype_size(dt);
  const bool has_src = op != LFA_ATOMIC_READ;
  int rc = lfa__iov_fetch_check(dst, src, has_src, nullptr, 0, res, nseg, esz);
  if (rc) return rc;
  IovTable &t = t_iov;
  t.reset(LFA_IOV_RW_NIN);
  size_t only = 0;
  for (size_t i = 0; i < nseg; i++) {
    if (!dst[i].count) continue;
    // ATOMIC_READ has no src: dst stands in its word, as launch_readwrite
    // measures the path over (dst, res, dst)
    const void *in[LFA_IOV_RW_NIN];
    in[LFA_IOV_RW_SRC - LFA_IOV_IN] = has_src ? src[i].addr : dst[i].addr;
    in[LFA_IOV_RW_RES - LFA_IOV_IN] = res[i].addr;
    if ((rc = t.add(dst[i].addr, dst[i].count, in, esz))) return rc;
    only = i;
  }
  if (!t.nseg()) return 0;
  // One segment is what lfa_atomic_readwrite_async takes: its launcher chooses
  // the tapered and nt-drained bodies by size, which a 256 MiB segment keeps.
  if (t.nseg() == 1)
    return kOps[op]->readwrite(dt, dst[only].addr, has_src ? src[only].addr : nullptr,
                               res[only].addr, dst[only].count, stream, 0);
  return iov_launch(t, stream, [&](const lfa_iov_args *a, unsigned ntile) {
    return kOps[op]->readwritev(dt, a, ntile, stream);
  });
}

int lfa_atomic_swapv_async(enum lfa_op op, enum lfa_datatype dt, const struct lfa_ioc *dst,
                           const struct lfa_ioc *src, const struct lfa_ioc *cmp,
                           const struct lfa_ioc *res, size_t nseg, void *stream) {
  if (op < LFA_CSWAP || op > LFA_MSWAP || (unsigned)dt >= LFA_DATATYPE_CNT ||
      !in_swap_table(op, dt))
    return -LFA_EOPNOTSUPP;
  if (!nseg) return 0;
  const size_t esz = lfa_datatype_size(dt);
  int rc = lfa__iov_fetch_check(dst, src, 1, cmp, 1, res, nseg, esz);
  if (rc) return rc;
  IovTable &t = t_iov;
  t.reset(LFA_IOV_SWAP_NIN);
  size_t only = 0;
  for (size_t i = 0; i < nseg; i++) {
    if (!dst[i].count) continue;
    const void *in[LFA_IOV_SWAP_NIN];
    in[LFA_IOV_SWAP_SRC - LFA_IOV_IN] = src[i].addr;
    in[LFA_IOV_SWAP_CMP - LFA_IOV_IN] = cmp[i].addr;
    in[LFA_IOV_SWAP_RES - LFA_IOV_IN] = res[i].addr;
    if ((rc = t.add(dst[i].addr, dst[i].count, in, esz))) return rc;
    only = i;
  }
  if (!t.nseg()) return 0;
  if (t.nseg() == 1)
    return kOps[op]->swap(dt, dst[only].addr, src[only].addr, cmp[only].addr, res[only].addr,
                          dst[only].count, stream, 0);
  return iov_launch(t, stream, [&](const lfa_iov_args *a, unsigned ntile) {
    return kOps[op]->swapv(dt, a, ntile, stream);
  });
}

}  // extern "C"
