// lfa_capi.cpp — the public C ABI of liblfa.so (include/lfa_atomic.h).
//
// Host-only C++: argument validation, the synchronous [op][datatype] tables
// (write, fetch, compare), and dispatch to the per-op kernel objects built
// from lfa_combine.hip.  No CPU compute path exists: every combine runs on
// the GPU.  Beside it: lfa_valid.cpp (the ofi_atomic_valid restatement),
// lfa_stage.cpp (host buffers), lfa_iov.cpp (the list forms), lfa_param.cpp.
#include <hip/hip_runtime_api.h>
#include <stdio.h>

#include "lfa_capi_int.h"
#include "lfa_signal.h"

#define LFA_OPS(X)                                                         \
  X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) \
  X(14) X(15) X(16) X(17) X(18)

#define LFA_OP_DECL(N) extern "C" const lfa_op_launch lfa__op##N;
#define LFA_OP_REF(N) &lfa__op##N,
LFA_OPS(LFA_OP_DECL)
const lfa_op_launch *const kOps[LFA_MSWAP + 1] = {LFA_OPS(LFA_OP_REF)};
#undef LFA_OP_DECL
#undef LFA_OP_REF

namespace {

// Where an operand lives: the synchronous tables take what their caller has
// — prov/coll's REDUCE items hand over host memory (coll_coll.c:364, :1058),
// a GPU-resident caller device memory.  Pinned and registered host memory
// counts as host: a small bucket runs the host loop; above it
// lfa_atomic_write_staged combines it in place over PCIe (zero-copy).
enum { kDev = 1, kHost = 2 };

int ptr_kind(const void *p) {
  hipPointerAttribute_t a;
  if (!p) return kHost;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // unknown to HIP: plain host memory
    return kHost;
  }
  return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) ? kDev : kHost;
}

// First failure of a synchronous table call on this thread (lfa_atomic_last_error).
thread_local int t_last_error = 0;

inline void note_error(int rc) {
  if (rc && !t_last_error) t_last_error = rc < 0 ? rc : -LFA_EIO;
}

// The device tail of the three synchronous entries: the launcher returned rc;
// wait for the null stream and report under the family's name.
void sync_finish(const char *family, int op, int dt, int rc) {
  hipError_t e = hipStreamSynchronize(nullptr);
  if (rc || e != hipSuccess)
    fprintf(stderr, "lfa: %s op=%d dt=%d failed (%d, %s)\n", family, op, dt, rc,
            hipGetErrorString(e));
  note_error(rc ? rc : e != hipSuccess ? -LFA_EIO : 0);
}

template <int OP, int DT>
void sync_rw_entry(void *dst, const void *src, void *res, size_t cnt) {
  if (!cnt) return;  // the reference's loop over zero elements: nothing, no GPU call
  const int k = ptr_kind(dst) | ptr_kind(res) | (OP == LFA_ATOMIC_READ ? 0 : ptr_kind(src));
  if (k == kHost) {
    int rc = lfa_host_readwrite((lfa_op)OP, (lfa_datatype)DT, dst, src, res, cnt);
    if (rc) fprintf(stderr, "lfa: host fetch op=%d dt=%d failed (%d)\n", OP, DT, rc);
    note_error(rc);
    return;
  }
  if (k != kDev) {
    fprintf(stderr, "lfa: fetch op=%d dt=%d: mixed host/device operands\n", OP, DT);
    note_error(-LFA_EINVAL);
    return;
  }
  sync_finish("fetch", OP, DT, kOps[OP]->readwrite(DT, dst, src, res, cnt, nullptr, 0));
}

template <int OP, int DT>
void sync_swap_entry(void *dst, const void *src, const void *cmp, void *res,
                     size_t cnt) {
  if (!cnt) return;
  const int k = ptr_kind(dst) | ptr_kind(src) | ptr_kind(cmp) | ptr_kind(res);
  if (k == kHost) {
    int rc = lfa_host_swap((lfa_op)OP, (lfa_datatype)DT, dst, src, cmp, res, cnt);
    if (rc) fprintf(stderr, "lfa: host swap op=%d dt=%d failed (%d)\n", OP, DT, rc);
    note_error(rc);
    return;
  }
  if (k != kDev) {
    fprintf(stderr, "lfa: swap op=%d dt=%d: mixed host/device operands\n", OP, DT);
    note_error(-LFA_EINVAL);
    return;
  }
  sync_finish("swap", OP, DT, kOps[OP]->swap(DT, dst, src, cmp, res, cnt, nullptr, 0));
}

template <int OP, int DT>
void sync_entry(void *dst, const void *src, size_t cnt) {
  if (!cnt) return;
  const int k = ptr_kind(dst) | ptr_kind(src);
  if (k != kDev) {
    // host (or mixed) operands: the host loop for a small bucket, HBM
    // streaming above lfa_host_small_bytes() (SURVEY §7 small-bucket latency)
    int rc = k == kHost && cnt * lfa_datatype_size((lfa_datatype)DT) <= lfa_host_small_bytes()
                 ? lfa_host_write((lfa_op)OP, (lfa_datatype)DT, dst, src, cnt)
                 : lfa_atomic_write_staged((lfa_op)OP, (lfa_datatype)DT, dst, src, cnt, 0);
    if (rc) fprintf(stderr, "lfa: combine op=%d dt=%d (host operands) failed (%d)\n", OP, DT, rc);
    note_error(rc);
    return;
  }
  sync_finish("combine", OP, DT, kOps[OP]->write(DT, dst, src, cnt, nullptr, 0));
}

// A table's cell: the entry where the reference's table has one, else NULL.
template <int OP, int DT>
constexpr lfa_write_fn entry() {
  if constexpr (in_table(OP, DT)) return &sync_entry<OP, DT>;
  else return nullptr;
}

template <int OP, int DT>
constexpr lfa_readwrite_fn rw_entry() {
  if constexpr (in_rw_table(OP, DT)) return &sync_rw_entry<OP, DT>;
  else return nullptr;
}

template <int OP, int DT>
constexpr lfa_swap_fn swap_entry() {
  if constexpr (in_swap_table(OP, DT)) return &sync_swap_entry<OP, DT>;
  else return nullptr;
}

}  // namespace

// One row of a table: cell template E over the 16 datatype columns.
#define LFA_ROW(E, OP)                                                          \
  { E<OP, 0>(), E<OP, 1>(), E<OP, 2>(), E<OP, 3>(), E<OP, 4>(), E<OP, 5>(),     \
    E<OP, 6>(), E<OP, 7>(), E<OP, 8>(), E<OP, 9>(), E<OP, 10>(), E<OP, 11>(),   \
    E<OP, 12>(), E<OP, 13>(), E<OP, 14>(), E<OP, 15>() }

extern "C" {

lfa_write_fn const lfa_atomic_write_handlers[LFA_WRITE_OP_CNT][LFA_DATATYPE_CNT] = {
    LFA_ROW(entry, 0), LFA_ROW(entry, 1), LFA_ROW(entry, 2),  LFA_ROW(entry, 3),
    LFA_ROW(entry, 4), LFA_ROW(entry, 5), LFA_ROW(entry, 6),  LFA_ROW(entry, 7),
    LFA_ROW(entry, 8), LFA_ROW(entry, 9), LFA_ROW(entry, 10), LFA_ROW(entry, 11)};

lfa_readwrite_fn const
    lfa_atomic_readwrite_handlers[LFA_READWRITE_OP_CNT][LFA_DATATYPE_CNT] = {
        LFA_ROW(rw_entry, 0), LFA_ROW(rw_entry, 1), LFA_ROW(rw_entry, 2),
        LFA_ROW(rw_entry, 3), LFA_ROW(rw_entry, 4), LFA_ROW(rw_entry, 5),
        LFA_ROW(rw_entry, 6), LFA_ROW(rw_entry, 7), LFA_ROW(rw_entry, 8),
        LFA_ROW(rw_entry, 9), LFA_ROW(rw_entry, 10), LFA_ROW(rw_entry, 11)};

lfa_swap_fn const lfa_atomic_swap_handlers[LFA_SWAP_OP_CNT][LFA_DATATYPE_CNT] = {
    LFA_ROW(swap_entry, 12), LFA_ROW(swap_entry, 13), LFA_ROW(swap_entry, 14),
    LFA_ROW(swap_entry, 15), LFA_ROW(swap_entry, 16), LFA_ROW(swap_entry, 17),
    LFA_ROW(swap_entry, 18)};

int lfa_atomic_last_error(void) {
  int rc = t_last_error;
  t_last_error = 0;
  return rc;
}

// The write, tree, fetch and compare launches share their validation with the
// lfa__write_as, lfa__tree_as, lfa__readwrite_as and lfa__swap_as entries
// below, which differ only in passing as_bytes on.
static int write_as(enum lfa_op op, enum lfa_datatype dt, void *dst, const void *src,
                    size_t cnt, void *stream, size_t as_bytes) {
  if ((unsigned)op >= LFA_WRITE_OP_CNT || !reducible(op, dt))
    return -LFA_EOPNOTSUPP;
  if (cnt && (!dst || !src)) return -LFA_EINVAL;
  return kOps[op]->write(dt, dst, src, cnt, stream, as_bytes);
}

static int tree_check(enum lfa_op op, enum lfa_datatype dt, void *dst,
                      const void *const *srcs, int nsrc, size_t cnt) {
  if ((unsigned)op > LFA_BXOR || !reducible(op, dt))
    return -LFA_EOPNOTSUPP;
  if (nsrc < 1 || nsrc > LFA_TREE_MAX || !srcs || (cnt && !dst))
    return -LFA_EINVAL;
  for (int k = 0; k < nsrc; k++)
    if (cnt && !srcs[k]) return -LFA_EINVAL;
  return 0;
}

int lfa_atomic_write_async(enum lfa_op op, enum lfa_datatype dt, void *dst,
                           const void *src, size_t cnt, void *stream) {
  return write_as(op, dt, dst, src, cnt, stream, 0);
}

static int readwrite_as(enum lfa_op op, enum lfa_datatype dt, void *dst, const void *src,
                        void *res, size_t cnt, void *stream, size_t as_bytes) {
  if ((unsigned)op >= LFA_READWRITE_OP_CNT || (unsigned)dt >= LFA_DATATYPE_CNT ||
      !in_rw_table(op, dt))
    return -LFA_EOPNOTSUPP;
  if (cnt && (!dst || !res || (op != LFA_ATOMIC_READ && !src)))
    return -LFA_EINVAL;
  return kOps[op]->readwrite(dt, dst, src, res, cnt, stream, as_bytes);
}

static int swap_as(enum lfa_op op, enum lfa_datatype dt, void *dst, const void *src,
                   const void *cmp, void *res, size_t cnt, void *stream, size_t as_bytes) {
  if (op < LFA_CSWAP || op > LFA_MSWAP || (unsigned)dt >= LFA_DATATYPE_CNT ||
      !in_swap_table(op, dt))
    return -LFA_EOPNOTSUPP;
  if (cnt && (!dst || !src || !cmp || !res)) return -LFA_EINVAL;
  return kOps[op]->swap(dt, dst, src, cmp, res, cnt, stream, as_bytes);
}

int lfa_atomic_readwrite_async(enum lfa_op op, enum lfa_datatype dt, void *dst,
                               const void *src, void *res, size_t cnt,
                               void *stream) {
  return readwrite_as(op, dt, dst, src, res, cnt, stream, 0);
}

int lfa_atomic_swap_async(enum lfa_op op, enum lfa_datatype dt, void *dst,
                          const void *src, const void *cmp, void *res,
                          size_t cnt, void *stream) {
  return swap_as(op, dt, dst, src, cmp, res, cnt, stream, 0);
}

int lfa_reduce_tree_async(enum lfa_op op, enum lfa_datatype dt, void *dst,
                          const void *const *srcs, int nsrc, size_t cnt,
                          void *stream) {
  if (int rc = tree_check(op, dt, dst, srcs, nsrc, cnt)) return rc;
  // One input is a copy (a one-member group's allreduce): from 16 MiB the
  // write table's ATOMIC_WRITE body beats hipMemcpyAsync D2D (83.3 vs 98.8 us
  // at 256 MiB, profiles/r02_probe_copy.log); below, the tree launcher's
  // hipMemcpyAsync stays.
  const size_t bytes = cnt * lfa_reduce_datatype_size(dt);
  if (nsrc == 1 && dst != srcs[0] && bytes >= ((size_t)16 << 20))
    return lfa_atomic_write_async(LFA_ATOMIC_WRITE, LFA_UINT8, dst, srcs[0], bytes,
                                  stream);
  return kOps[op]->tree(dt, dst, srcs, nsrc, cnt, stream, 0);
}

// Test-only entries (internal, as lfa__tune_* in liblfa_tune.so; not in
// include/lfa_atomic.h): the write, tree, fetch and compare calls above with
// the vector body's form chosen as if the body were `as_bytes` bytes
// (lfa_split.h; 0: by the real size), so that tests/test_sweep_forms_gpu.py
// runs every form those launchers only take from 32, 64 or 192 MiB on a 40 or
// 50 KiB buffer.  The tree entry goes to the tree launcher whatever nsrc is.
int lfa__write_as(int op, int dt, void *dst, const void *src, size_t cnt, void *stream,
                  size_t as_bytes) {
  return write_as((lfa_op)op, (lfa_datatype)dt, dst, src, cnt, stream, as_bytes);
}

int lfa__tree_as(int op, int dt, void *dst, const void *const *srcs, int nsrc, size_t cnt,
                 void *stream, size_t as_bytes) {
  if (int rc = tree_check((lfa_op)op, (lfa_datatype)dt, dst, srcs, nsrc, cnt)) return rc;
  return kOps[op]->tree(dt, dst, srcs, nsrc, cnt, stream, as_bytes);
}

int lfa__readwrite_as(int op, int dt, void *dst, const void *src, void *res, size_t cnt,
                      void *stream, size_t as_bytes) {
  return readwrite_as((lfa_op)op, (lfa_datatype)dt, dst, src, res, cnt, stream, as_bytes);
}

int lfa__swap_as(int op, int dt, void *dst, const void *src, const void *cmp, void *res,
                 size_t cnt, void *stream, size_t as_bytes) {
  return swap_as((lfa_op)op, (lfa_datatype)dt, dst, src, cmp, res, cnt, stream, as_bytes);
}

int lfa_reduce_tree_put_async(enum lfa_op op, enum lfa_datatype dt,
                              void *const *dsts, int ndst, const void *const *srcs,
                              int nsrc, size_t cnt, void *stream) {
  if ((unsigned)op > LFA_BXOR || !reducible(op, dt))
    return -LFA_EOPNOTSUPP;
  if (nsrc < 1 || nsrc > LFA_TREE_MAX || !srcs || ndst < 1 || ndst > LFA_PUT_MAX ||
      !dsts)
    return -LFA_EINVAL;
  for (int k = 0; k < nsrc; k++)
    if (cnt && !srcs[k]) return -LFA_EINVAL;
  for (int j = 0; j < ndst; j++)
    if (cnt && !dsts[j]) return -LFA_EINVAL;
  return kOps[op]->treeput(dt, dsts, ndst, srcs, nsrc, cnt, stream);
}

// The one-shot launch shares its validation with the lfa__oneshot_as entry
// below, which differs only in passing ll on.
static int oneshot_as(int op, int dt, const struct lfa_oneshot *a, void *stream, int ll) {
  if ((unsigned)op > LFA_BXOR || !reducible(op, dt))
    return -LFA_EOPNOTSUPP;
  if (!a) return -LFA_EINVAL;
  return kOps[op]->oneshot(dt, a, stream, ll);
}

int lfa_oneshot_reduce_async(int op, int dt, const struct lfa_oneshot *a,
                                void *stream) {
  return oneshot_as(op, dt, a, stream, -1);
}

// Test-only entry (internal, as lfa__write_as; not in include/): the one-shot
// launch with the kernel chosen per call instead of by LFA_OS_LL, which a
// process reads once, so that tests/test_sweep_oneshot_gpu.py runs both
// kernels in one process.  ll < 0: the launcher's own choice; 0: the flagged
// kernel; 1: the LL kernel, or -LFA_EINVAL where the launcher's rule forbids it
// apart from the environment (one member, a part above LFA_OS_LL_BYTES, reduce
// to a root): never a silent fall-back.
int lfa__oneshot_as(int op, int dt, const struct lfa_oneshot *a, void *stream, int ll) {
  return oneshot_as(op, dt, a, stream, ll < 0 ? -1 : ll > 0);
}

}  // extern "C"
