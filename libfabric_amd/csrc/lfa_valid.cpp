// lfa_valid.cpp — the reference's validity and size tables (ofi_atomic_valid,
// ofi_datatype_size) and their reducing variants.  Arithmetic on enums: no
// HIP, so a host-only program can link it (tools/iov_host_check.cpp).  The
// membership predicates themselves are in lfa_capi_int.h.
#include <errno.h>

#include "lfa_capi_int.h"

extern "C" {

size_t lfa_datatype_size(enum lfa_datatype dt) {
  static const size_t sz[LFA_DATATYPE_CNT] = {1, 1, 2, 2, 4, 4, 8, 8,
                                              4, 8, 8, 16, 16, 32, 16, 16};
  if ((unsigned)dt >= LFA_DATATYPE_CNT) {
    errno = EINVAL;
    return 0;
  }
  return sz[dt];
}

int lfa_atomic_valid(enum lfa_datatype dt, enum lfa_op op, uint64_t flags) {
  if (flags & LFA_TAGGED) {
    if (flags & (LFA_FETCH_ATOMIC | LFA_COMPARE_ATOMIC)) return -LFA_ENOSYS;
  } else if (flags & ~(LFA_FETCH_ATOMIC | LFA_COMPARE_ATOMIC)) {
    return -LFA_EBADFLAGS;
  } else if ((flags & LFA_FETCH_ATOMIC) && (flags & LFA_COMPARE_ATOMIC)) {
    return -LFA_EBADFLAGS;
  }
  if ((unsigned)dt >= LFA_DATATYPE_CNT) return -LFA_EOPNOTSUPP;
  if (flags & LFA_FETCH_ATOMIC)
    return (unsigned)op < LFA_READWRITE_OP_CNT && in_rw_table(op, dt)
               ? 0 : -LFA_EOPNOTSUPP;
  if (flags & LFA_COMPARE_ATOMIC)
    return in_swap_table(op, dt) ? 0 : -LFA_EOPNOTSUPP;
  if ((unsigned)op >= LFA_WRITE_OP_CNT || op == LFA_ATOMIC_READ)
    return -LFA_EOPNOTSUPP;
  return in_table(op, dt) ? 0 : -LFA_EOPNOTSUPP;
}

size_t lfa_reduce_datatype_size(enum lfa_datatype dt) {
  if (is_half(dt)) return 2;
  return lfa_datatype_size(dt);
}

int lfa_reduce_valid(enum lfa_datatype dt, enum lfa_op op) {
  if (!is_half(dt)) return lfa_atomic_valid(dt, op, 0);
  return (unsigned)op < LFA_WRITE_OP_CNT && reducible(op, dt) ? 0 : -LFA_EOPNOTSUPP;
}

}  // extern "C"
