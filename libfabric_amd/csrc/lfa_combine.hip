// lfa_combine.hip — MI355X (gfx950) combine kernels + their C ABI (liblfa.so).
//
// What runs on the GPU for libfabric's L4 combine layer
// (ofi_atomic_write_handlers, prov/util/src/util_atomic.c:907-922, called by
// prov/coll's REDUCE items, prov/coll/src/coll_coll.c:758-768):
//
//   combine_lds    dst[i] = dst[i] OP src[i] over 16-byte vectors (the product
//                  body).  A pure HBM stream (2 reads + 1 write per element,
//                  ~0.1 op/B): no MFMA — the roofline is HBM.  Each
//                  wave DMAs 4 KiB of each operand into LDS (global_load_lds,
//                  nt), reads it back with ds_read_b128, applies OP and stores
//                  nt; every wave-instruction moves 1 KiB of consecutive bytes.
//                  One tile body, lds_tile, which combine_lds_taper (short
//                  tiles for the last workgroups) and combine_iov share.
//   combine_elem   the same op for misaligned heads/tails and for buffers that
//                  are not co-aligned mod 16 (one element per lane, coalesced).
//   reduce_tree_*  N inputs → 1 output in ONE pass, in prov/coll's
//                  recursive-doubling association order (coll_coll.c:349-449):
//                  replaces log2(N) pairwise REDUCE+COPY items, traffic
//                  (N+1)·S instead of ~3·log2(N)·S.
//   reduce_tree_put the same tree with its result written to several
//                  outputs, every access system scope: the LFA_ALGO_P2P kernel
//                  that reads peers' HBM and pushes into it over xGMI.
//   fetch_lds/elem the fetch (readwrite) and compare-swap tables
//                  (util_atomic.c:924-980): res = old dst, then the update;
//                  fetch_lds and fetch_lds_taper over one tile body, fetch_tile.
//   combine_iov, reduce_iov, fetch_iov  the list (fi_ioc) forms: every segment
//                  of a call in one launch (lfa_k_iov.hpp).
//
// Kernels and launchers: lfa_kernels.hpp (how a buffer is cut into head,
// vectors and tail: lfa_split.h).  The forms only the tuning library builds:
// lfa_tune_forms.hpp, not included here.  Semantics: lfa_ops.hpp.  Build: hipcc --offload-arch=gfx950 -O3
// -ffp-contract=off -DLFA_OP=<op>, once per enum fi_op row (0..18; see
// libfabric_amd/build.py).
#include "lfa_kernels.hpp"
#include "lfa_launch.h"

namespace lfa {

// ---------------------------------------------------------------------------
// per-op entry points
// ---------------------------------------------------------------------------
// This file is compiled once per write op (-DLFA_OP=<enum fi_op value>) so the
// ~100 (op, datatype) kernel families build in parallel; each object exports
// one record, lfa__op<N> (struct lfa_op_launch, lfa_launch.h): the launch
// entries of the forms op N has, NULL for the others.  lfa_capi.cpp gathers
// the 19 records in kOps and dispatches through them.  The entries return 0
// or a negative LFA_E* code.
// Ops whose result bits do not depend on an integer's signedness: wrapping
// SUM / PROD (the low bits of a two's-complement sum or product), the
// bitwise and logical ops, READ / WRITE, CSWAP (bitwise compare), CSWAP_NE
// (integer != is sign-blind) and MSWAP.  A signed integer type runs its
// unsigned twin's kernels for them — the same bits, one kernel family
// instead of two (liblfa.so size).  MIN / MAX and the
// ordered compares keep their own.
template <int OP>
constexpr bool sign_blind() {
  return !(OP == OP_MIN || OP == OP_MAX || OP == OP_CSWAP_LE || OP == OP_CSWAP_LT ||
           OP == OP_CSWAP_GE || OP == OP_CSWAP_GT);
}

// the kernel type of a signed integer under OP: its unsigned twin when OP
// is sign-blind (if constexpr: the signed family is never instantiated)
template <int OP, typename S, typename U, typename F>
static int signed_case(F &&f) {
  if constexpr (sign_blind<OP>()) return f((U *)0);
  else return f((S *)0);
}

template <int OP, typename F>
static int by_type(int dt, F &&f) {
  switch (dt) {
    case LFA_INT8: return signed_case<OP, int8_t, uint8_t>(f);
    case LFA_UINT8: return f((uint8_t *)0);
    case LFA_INT16: return signed_case<OP, int16_t, uint16_t>(f);
    case LFA_UINT16: return f((uint16_t *)0);
    case LFA_INT32: return signed_case<OP, int32_t, uint32_t>(f);
    case LFA_UINT32: return f((uint32_t *)0);
    case LFA_INT64: return signed_case<OP, int64_t, uint64_t>(f);
    case LFA_UINT64: return f((uint64_t *)0);
    case LFA_FLOAT: return f((float *)0);
    case LFA_DOUBLE: return f((double *)0);
    case LFA_FLOAT_COMPLEX: return f((cf32 *)0);
    case LFA_INT128: return signed_case<OP, i128, u128>(f);
    case LFA_UINT128: return f((u128 *)0);
    default: return -LFA_EOPNOTSUPP;
  }
}

// The reducing entry points (write, tree, tree-put, one-shot) also take
// FI_FLOAT16 / FI_BFLOAT16 (lfa_reduce_valid); the fetch and compare tables
// do not.  ATOMIC_WRITE moves 16-bit patterns: the uint16_t kernels.
template <int OP, typename F>
static int by_reduce_type(int dt, F &&f) {
  switch (dt) {
    case LFA_FLOAT16:
      if constexpr (OP == OP_WRITE) return f((uint16_t *)0);
      else return f((f16 *)0);
    case LFA_BFLOAT16:
      if constexpr (OP == OP_WRITE) return f((uint16_t *)0);
      else return f((bf16 *)0);
    default: return by_type<OP>(dt, f);
  }
}

// The list forms (lfa_k_iov.hpp): one kernel family per (op, element type)
// on top of the sharing above.  ATOMIC_WRITE only moves bytes, so it runs the
// unsigned integer of the element's width whatever the datatype.
template <int OP, typename F>
static int by_iov_type(int dt, F &&f) {
  if constexpr (OP == OP_WRITE) {
    switch (lfa_reduce_datatype_size((lfa_datatype)dt)) {
      case 1: return f((uint8_t *)0);
      case 2: return f((uint16_t *)0);
      case 4: return f((uint32_t *)0);
      case 8: return f((uint64_t *)0);
      case 16: return f((u128 *)0);
      default: return -LFA_EOPNOTSUPP;
    }
  } else {
    return by_reduce_type<OP>(dt, f);
  }
}

// The fetch and compare list forms: ATOMIC_READ and ATOMIC_WRITE (an exchange)
// only move bytes, so they run the unsigned integer of the element's width
// whatever the datatype; every other op shares as the contiguous tables do.
template <int OP, typename F>
static int by_iov_fetch_type(int dt, F &&f) {
  if constexpr (OP == OP_READ || OP == OP_WRITE) {
    if ((unsigned)dt >= LFA_DATATYPE_CNT) return -LFA_EOPNOTSUPP;
    switch (lfa_datatype_size((lfa_datatype)dt)) {
      case 1: return f((uint8_t *)0);
      case 2: return f((uint16_t *)0);
      case 4: return f((uint32_t *)0);
      case 8: return f((uint64_t *)0);
      case 16: return f((u128 *)0);
      default: return -LFA_EOPNOTSUPP;
    }
  } else {
    return by_type<OP>(dt, f);
  }
}

}  // namespace lfa

#ifndef LFA_OP
#error "compile with -DLFA_OP=<op>"
#endif

#define LFA_CAT2(a, b) a##b
#define LFA_CAT(a, b) LFA_CAT2(a, b)

// Which forms op LFA_OP has: each is a function where it does, and a null
// pointer of the member's type where it does not.
#if LFA_OP <= 11 && LFA_OP != 10
static int op_write(int dt, void *dst, const void *src, size_t cnt, void *stream,
                    size_t as_bytes) {
  // dt | LFA_WRITE_MAPPED: operands on their host mappings (lfa_stage.cpp)
  const bool mapped = (dt & LFA_WRITE_MAPPED) != 0;
  return lfa::by_reduce_type<LFA_OP>(dt & ~LFA_WRITE_MAPPED, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_write<LFA_OP, T>(dst, src, cnt, (hipStream_t)stream, mapped, as_bytes);
  });
}

static int op_writev(int dt, const lfa_iov_args *a, unsigned ntile, void *stream) {
  return lfa::by_iov_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_writev<LFA_OP, T>(*a, ntile, (hipStream_t)stream);
  });
}
#else
constexpr lfa_launch_write_t op_write = nullptr;
constexpr lfa_launch_writev_t op_writev = nullptr;
#endif

#if LFA_OP <= 9
static int op_treev(int dt, const lfa_iov_args *a, int nsrc, unsigned ntile,
                    void *stream) {
  return lfa::by_reduce_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_treev<LFA_OP, T>(*a, nsrc, ntile, (hipStream_t)stream);
  });
}

static int op_tree(int dt, void *dst, const void *const *srcs, int nsrc, size_t cnt,
                   void *stream, size_t as_bytes) {
  return lfa::by_reduce_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_tree<LFA_OP, T>(dst, srcs, nsrc, cnt, (hipStream_t)stream, -1,
                                       as_bytes);
  });
}

static int op_oneshot(int dt, const lfa_oneshot *a, void *stream, int ll) {
  return lfa::by_reduce_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_oneshot<LFA_OP, T>(*a, (hipStream_t)stream, ll);
  });
}

static int op_treeput(int dt, void *const *dsts, int ndst, const void *const *srcs,
                      int nsrc, size_t cnt, void *stream) {
  return lfa::by_reduce_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_tree_put<LFA_OP, T>(dsts, ndst, srcs, nsrc, cnt,
                                           (hipStream_t)stream);
  });
}
#else
constexpr lfa_launch_treev_t op_treev = nullptr;
constexpr lfa_launch_tree_t op_tree = nullptr;
constexpr lfa_launch_oneshot_t op_oneshot = nullptr;
constexpr lfa_launch_treeput_t op_treeput = nullptr;
#endif

#if LFA_OP <= 11
static int op_readwrite(int dt, void *dst, const void *src, void *res, size_t cnt,
                        void *stream, size_t as_bytes) {
  return lfa::by_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_readwrite<LFA_OP, T>(dst, src, res, cnt,
                                            (hipStream_t)stream, as_bytes);
  });
}
static int op_readwritev(int dt, const lfa_iov_args *a, unsigned ntile, void *stream) {
  return lfa::by_iov_fetch_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_readwritev<LFA_OP, T>(*a, ntile, (hipStream_t)stream);
  });
}
constexpr lfa_launch_swap_t op_swap = nullptr;
constexpr lfa_launch_fetchv_t op_swapv = nullptr;
#else
constexpr lfa_launch_readwrite_t op_readwrite = nullptr;
constexpr lfa_launch_fetchv_t op_readwritev = nullptr;
static int op_swap(int dt, void *dst, const void *src, const void *cmp, void *res,
                   size_t cnt, void *stream, size_t as_bytes) {
  return lfa::by_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_swap<LFA_OP, T>(dst, src, cmp, res, cnt,
                                       (hipStream_t)stream, as_bytes);
  });
}

static int op_swapv(int dt, const lfa_iov_args *a, unsigned ntile, void *stream) {
  return lfa::by_type<LFA_OP>(dt, [&](auto *tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    return lfa::launch_swapv<LFA_OP, T>(*a, ntile, (hipStream_t)stream);
  });
}
#endif

// host data: the device pass would emit a const object too, and has no entries
#ifndef __HIP_DEVICE_COMPILE__
extern "C" const lfa_op_launch LFA_CAT(lfa__op, LFA_OP) = {
    op_write,   op_writev,    op_tree, op_treev,      op_treeput,
    op_oneshot, op_readwrite, op_swap, op_readwritev, op_swapv};
#endif
