/* lfa_iov.h — the segment table of the list (fi_ioc) forms, shared by the
 * host side that builds it (lfa_iov_table.h) and the kernels that walk it
 * (lfa_k_iov.hpp).  Plain C: no HIP types.
 *
 * One launch covers every non-empty segment of a call.  The host cuts each
 * segment into tiles of LFA_IOV_TILE bytes of dst and numbers the tiles
 * through all segments; workgroup b owns tile b.  The table is an array of
 * 64-bit words:
 *
 *   words [0, P)            uint32_t first_tile[nseg + 1], the prefix sum of
 *                           the segments' tile counts (first_tile[nseg] is the
 *                           grid), P = (nseg + 2) / 2
 *   words [P + s·R, …)      segment s: dst, count (elements), in[0 .. nin)
 *                           R = 2 + nin; nin = 1 for writev (src), nsrc for
 *                           treev, 2 for readwritev (src, res), 3 for swapv
 *                           (src, cmp, res)
 *
 * The fetch and compare forms write `res` too; it is a pointer of the record
 * like the inputs (the last one), and the kernels reach every word of a
 * record through the LFA_IOV_* indices below.
 *
 * A table of at most LFA_IOV_INLINE words travels in the kernel arguments
 * (`inl`, tab == NULL); a larger one is copied to a device ring slot that
 * `tab` names.
 */
#ifndef LFA_IOV_H
#define LFA_IOV_H

#include <stddef.h>
#include <stdint.h>

#include "lfa_split.h"

#define LFA_IOV_TILE 16384u /* bytes of dst per workgroup: 4 KiB per wave */
#define LFA_IOV_INLINE 64   /* words: 512 bytes of kernel arguments */
#define LFA_IOV_TREE_LEAVES 8 /* the fused tree form's widest kernel: 2..15 inputs */

struct lfa_iov_args {
  const uint64_t *tab; /* device table, or NULL: the table is `inl` */
  uint32_t nseg;       /* non-empty segments */
  uint32_t nin;        /* inputs per segment */
  uint32_t direct;     /* every segment is one tile: workgroup b owns segment b */
  uint32_t pad;
  uint64_t inl[LFA_IOV_INLINE];
};

/* Words of a record, from its first: dst, count, then the further pointers. */
#define LFA_IOV_DST 0
#define LFA_IOV_COUNT 1
#define LFA_IOV_IN 2 /* in[k] is word LFA_IOV_IN + k */
/* the further pointers of the fetch (nin = 2) and compare (nin = 3) records */
#define LFA_IOV_RW_NIN 2
#define LFA_IOV_RW_SRC (LFA_IOV_IN + 0)
#define LFA_IOV_RW_RES (LFA_IOV_IN + 1)
#define LFA_IOV_SWAP_NIN 3
#define LFA_IOV_SWAP_SRC (LFA_IOV_IN + 0)
#define LFA_IOV_SWAP_CMP (LFA_IOV_IN + 1)
#define LFA_IOV_SWAP_RES (LFA_IOV_IN + 2)

#define LFA_IOV_FN LFA_SPLIT_FN

LFA_IOV_FN size_t lfa_iov_prefix_words(size_t nseg) { return (nseg + 2) / 2; }

/* Tiles of a segment of `count` elements of `esz` bytes (esz divides 16)
 * whose operands' addresses OR to `any`.
 * Operands not aligned to the element: tiles of LFA_IOV_TILE / esz elements
 * from element 0.  Otherwise the elements before dst's first 16-byte boundary
 * (the head, lfa_split_head) belong to tile 0 and the tiles start at that boundary, so every
 * tile boundary inside a segment is a 16-byte boundary of dst. */
LFA_IOV_FN size_t lfa_iov_tiles(uintptr_t dst, uintptr_t any, size_t count, size_t esz) {
  const size_t rest = any % esz ? count : count - lfa_split_head(dst, count, esz);
  const size_t n = (rest * esz + LFA_IOV_TILE - 1) / LFA_IOV_TILE;
  return n ? n : 1;
}

#endif /* LFA_IOV_H */
