/* lfa_split.h — how one buffer of a call is cut up, in one place: the path its
 * operands' addresses permit, the head / vector body / tail of the vector
 * path, and the tapered grid of a vector body.  Shared by every launcher
 * (lfa_k_launch.hpp), the list kernels and their host side (lfa_iov.h) and
 * the tuning library.  Plain C: no HIP types.
 */
#ifndef LFA_SPLIT_H
#define LFA_SPLIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LFA_SPLIT_FN __host__ __device__ static inline
#else
#define LFA_SPLIT_FN static inline
#endif

enum lfa_path {
  LFA_PATH_BYTES, /* some operand not aligned to the element: byte-wise moves */
  LFA_PATH_ELEM,  /* aligned to the element, not co-aligned: one element per lane */
  LFA_PATH_VEC    /* every operand co-aligned mod 16 and esz <= 16: 16-byte vectors */
};

/* The path of a call over its outputs and inputs (esz a power of two);
 * outs[0] is the operand the others are measured against and the one whose
 * 16-byte boundaries cut the vectors. */
LFA_SPLIT_FN enum lfa_path lfa_split_path(const void *const *outs, int nout,
                                          const void *const *ins, int nin, size_t esz) {
  const uintptr_t p0 = (uintptr_t)outs[0];
  uintptr_t any = 0, mis = 0;
  for (int k = 0; k < nout; k++) {
    any |= (uintptr_t)outs[k];
    mis |= (uintptr_t)outs[k] ^ p0;
  }
  for (int k = 0; k < nin; k++) {
    any |= (uintptr_t)ins[k];
    mis |= (uintptr_t)ins[k] ^ p0;
  }
  if (any % esz) return LFA_PATH_BYTES;
  return mis % 16 == 0 && esz <= 16 ? LFA_PATH_VEC : LFA_PATH_ELEM;
}

/* The elements before dst's first 16-byte boundary, at most `count`. */
LFA_SPLIT_FN size_t lfa_split_head(uintptr_t dst, size_t count, size_t esz) {
  size_t head = ((16 - dst % 16) % 16) / esz;
  return head < count ? head : count;
}

/* count = head + body + tail elements: `head` before dst's first 16-byte
 * boundary, `body` in nvec whole vectors, `tail` after the last of them.  Off
 * the vector path there are no vectors and every element is head. */
struct lfa_split {
  size_t head, nvec, body, tail;
};

LFA_SPLIT_FN struct lfa_split lfa_split_of(enum lfa_path path, uintptr_t dst, size_t count,
                                           size_t esz) {
  struct lfa_split s;
  s.head = path == LFA_PATH_VEC ? lfa_split_head(dst, count, esz) : count;
  s.nvec = (count - s.head) * esz / 16;
  s.body = s.nvec * 16 / esz;
  s.tail = count - s.head - s.body;
  return s;
}

/* A tapered grid over nvec vectors: the first nhead workgroups take hv
 * vectors each up to vector `split` (a multiple of hv, so every head tile is
 * whole), and ntail workgroups of tv vectors cover the last 1/div or so. */
struct lfa_taper {
  size_t split;
  unsigned nhead, ntail;
};

LFA_SPLIT_FN struct lfa_taper lfa_split_taper(size_t nvec, size_t div, size_t hv, size_t tv) {
  struct lfa_taper t;
  t.split = nvec - nvec / div;
  t.split -= t.split % hv;
  t.nhead = (unsigned)(t.split / hv);
  t.ntail = (unsigned)((nvec - t.split + tv - 1) / tv);
  return t;
}

#endif /* LFA_SPLIT_H */
