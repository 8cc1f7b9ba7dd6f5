/* lfa_split.h — how one buffer of a call is cut up, in one place: the path its
 * operands' addresses permit, the head / vector body / tail of the vector
 * path, the tapered grid of a vector body, and the form of that body a
 * launcher picks by size (lfa_form_write, lfa_form_tree, lfa_form_fetch).  Shared by every launcher
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

/* Which form of a vector body launch_write, launch_tree_body and launch_fetch run, by the body's size in bytes
 * per operand (nvec * 16).  The launchers (lfa_k_launch.hpp) switch on these
 * and on nothing else; the measurements behind every threshold are quoted
 * there.  Pure functions of their arguments: tools/split_host_check.cpp
 * prints them around every threshold. */
#define LFA_TAPER_BYTES ((size_t)32 << 20)       /* write: tapered tail from here */
#define LFA_SC1_BYTES ((size_t)192 << 20)        /* below: write-through stores; from here: nt */

/* A launcher's `as_bytes` argument: 0 chooses by the real body, anything
 * else as if the body were that many bytes.  Only the form follows it; the
 * split, the grid and the kernel arguments come from the real size.  The
 * product passes 0; the lfa__write_as / lfa__tree_as / lfa__readwrite_as /
 * lfa__swap_as entries (lfa_capi.cpp) let the tests run every large-size
 * form on a small buffer. */
LFA_SPLIT_FN size_t lfa_form_bytes(size_t nvec, size_t as_bytes) {
  return as_bytes ? as_bytes : nvec * 16;
}

enum lfa_write_form {
  LFA_WRITE_SC1,   /* combine_lds, write-through stores */
  LFA_WRITE_TAPER, /* combine_lds_taper, write-through stores */
  LFA_WRITE_NT     /* combine_lds, nt stores, drained (combine_drain) */
};

/* mapped: host-mapped operands (lfa_atomic_write_staged's zero-copy form). */
LFA_SPLIT_FN enum lfa_write_form lfa_form_write(size_t body_bytes, int mapped) {
  if (mapped) return LFA_WRITE_SC1;
  if (body_bytes >= LFA_SC1_BYTES) return LFA_WRITE_NT;
  return body_bytes >= LFA_TAPER_BYTES ? LFA_WRITE_TAPER : LFA_WRITE_SC1;
}

/* The tree's vector body, under the numbers bench.py --tune-tree gives the
 * forms: reduce_tree_chunk<.., 1> (1) and <.., 2> (2) with nt stores,
 * reduce_tree_lds (3), reduce_tree_chunk<.., 2> with write-through stores
 * (11), reduce_tree_put's body with one output (25). */
enum {
  LFA_TREE_CHUNK1 = 1,
  LFA_TREE_CHUNK2 = 2,
  LFA_TREE_LDS = 3,
  LFA_TREE_CHUNK2_SC1 = 11,
  LFA_TREE_PUT = 25
};

struct lfa_tree_form {
  int variant;
  int cap_lds; /* LFA_TREE_CHUNK2_SC1 only: launch with the 41 KiB of idle LDS */
};

/* nsrc in [nleaf, 2 * nleaf), nleaf a power of two, esz the element size. */
LFA_SPLIT_FN struct lfa_tree_form lfa_form_tree(size_t body_bytes, int nsrc, int nleaf,
                                                size_t esz) {
  struct lfa_tree_form f;
  f.cap_lds = 0;
  if (body_bytes >= LFA_SC1_BYTES) {
    f.variant = nsrc <= 2 ? LFA_TREE_LDS : nsrc > 8 ? LFA_TREE_CHUNK2 : LFA_TREE_CHUNK1;
  } else if (nleaf == 8 && esz >= 4) {
    f.variant = LFA_TREE_PUT;
  } else {
    f.variant = LFA_TREE_CHUNK2_SC1;
    f.cap_lds = nsrc >= 3 && nsrc <= 8;
  }
  return f;
}

/* The fetch and compare tables' vector body (launch_fetch), by the body's
 * size per operand and the functor's inputs (nin: 1 ATOMIC_READ, 2 the other
 * readwrite ops, 3 the compare table):
 *
 *   below LFA_FETCH_TAPER_BYTES   fetch_lds, write-through, drained iff nin == 2
 *   from LFA_FETCH_TAPER_BYTES    nin == 2 only: fetch_lds_taper, write-through
 *   from LFA_SC1_BYTES            every nin: fetch_lds_taper, nt stores
 */
#define LFA_FETCH_TAPER_BYTES ((size_t)64 << 20) /* two-input fetch: tapered tail from here */

enum lfa_fetch_form {
  LFA_FETCH_LDS,       /* fetch_lds, write-through stores */
  LFA_FETCH_TAPER_SC1, /* fetch_lds_taper, write-through stores */
  LFA_FETCH_TAPER_NT   /* fetch_lds_taper, nt stores */
};

LFA_SPLIT_FN enum lfa_fetch_form lfa_form_fetch(size_t body_bytes, int nin) {
  if (body_bytes >= LFA_SC1_BYTES) return LFA_FETCH_TAPER_NT;
  return nin == 2 && body_bytes >= LFA_FETCH_TAPER_BYTES ? LFA_FETCH_TAPER_SC1 : LFA_FETCH_LDS;
}

#endif /* LFA_SPLIT_H */
