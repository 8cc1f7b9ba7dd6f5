// lfa_capi_int.h — what the units of liblfa.so's C ABI share (lfa_capi.cpp,
// lfa_valid.cpp, lfa_stage.cpp, lfa_iov.cpp): the reference's table
// membership by enum, the per-op launch records and the device limit.
// No HIP types: lfa_valid.cpp compiles without the HIP headers.
#ifndef LFA_CAPI_INT_H
#define LFA_CAPI_INT_H

#include "../../include/lfa_atomic.h"
#include "lfa_launch.h"

// Table membership (util_atomic.c:907-922, HAVE_BUILTIN_MM_ATOMICS build with
// 128-bit atomics): REALNO = int8..double + int128; ALL = REALNO + float
// complex; INT = int8..uint64 + int128.
constexpr bool in_table(int op, int dt) {
  const bool realno = dt <= LFA_DOUBLE || dt == LFA_INT128 || dt == LFA_UINT128;
  const bool all = realno || dt == LFA_FLOAT_COMPLEX;
  const bool ints = dt <= LFA_UINT64 || dt == LFA_INT128 || dt == LFA_UINT128;
  switch (op) {
    case LFA_MIN: case LFA_MAX: return realno;
    case LFA_SUM: case LFA_PROD: case LFA_LOR: case LFA_LAND: case LFA_LXOR:
    case LFA_ATOMIC_WRITE: return all;
    case LFA_BOR: case LFA_BAND: case LFA_BXOR: return ints;
    default: return false;
  }
}

// What the reducing entry points and the collectives take: the write table's
// members, and FI_FLOAT16 / FI_BFLOAT16 under the float column's write-row
// ops (lfa_ops.hpp).  The [op][LFA_DATATYPE_CNT] tables, lfa_atomic_valid and
// lfa_datatype_size keep the reference's 16 columns.
constexpr bool is_half(int dt) { return dt == LFA_FLOAT16 || dt == LFA_BFLOAT16; }
constexpr bool reducible(int op, int dt) {
  if (is_half(dt)) return in_table(op, LFA_FLOAT);
  return dt >= 0 && dt < LFA_DATATYPE_CNT && in_table(op, dt);
}

// Fetch table (util_atomic.c:924-950): the write rows plus an ALL-types
// ATOMIC_READ row; ATOMIC_WRITE is an exchange.
constexpr bool in_rw_table(int op, int dt) {
  return op == LFA_ATOMIC_READ ? in_table(LFA_ATOMIC_WRITE, dt) : in_table(op, dt);
}

// Compare table (util_atomic.c:952-980): CSWAP / CSWAP_NE over ALL types,
// LE/LT/GE/GT over REALNO, MSWAP over INT.
constexpr bool in_swap_table(int op, int dt) {
  switch (op) {
    case LFA_CSWAP: case LFA_CSWAP_NE: return in_table(LFA_SUM, dt);
    case LFA_CSWAP_LE: case LFA_CSWAP_LT: case LFA_CSWAP_GE: case LFA_CSWAP_GT:
      return in_table(LFA_MIN, dt);
    case LFA_MSWAP: return in_table(LFA_BOR, dt);
    default: return false;
  }
}

// The launch record of every op (lfa_launch.h), by enum lfa_op; lfa_capi.cpp.
// The guards above keep a call from a form its op does not have.
extern const lfa_op_launch *const kOps[LFA_MSWAP + 1] __attribute__((visibility("hidden")));

// per-device state (staging slots, list-form rings) is sized by this
constexpr int kMaxDevices = 64;

#endif  // LFA_CAPI_INT_H
