/* lfa_launch.h — the link between the C ABI's host units (lfa_capi.cpp,
 * lfa_stage.cpp, lfa_iov.cpp) and the 19 per-op objects built from
 * lfa_combine.hip.  Plain C: no HIP types.
 *
 * Each object exports one record, lfa__op<N>, whose members are its launch
 * entries; a form the op does not have is NULL.  Both sides take the
 * signatures from here.  Every entry returns 0 or a negative LFA_E* code;
 * `dt` is an enum lfa_datatype (write: | LFA_WRITE_MAPPED, lfa_signal.h),
 * `stream` a hipStream_t.  write, tree, readwrite and swap end in `as_bytes`:
 * 0 from every product caller; otherwise the vector body's form is chosen as
 * if the body were that many bytes (lfa_split.h; the lfa__write_as /
 * lfa__tree_as / lfa__readwrite_as / lfa__swap_as test entries).  oneshot ends in `ll`: -1 from every product caller (the
 * launcher's own choice of kernel); 0 the flagged kernel, 1 the LL kernel (the
 * lfa__oneshot_as test entry).
 */
#ifndef LFA_LAUNCH_H
#define LFA_LAUNCH_H

#include <stddef.h>

struct lfa_iov_args; /* lfa_iov.h */
struct lfa_oneshot;  /* lfa_signal.h */

typedef int (*lfa_launch_write_t)(int dt, void *dst, const void *src, size_t cnt, void *stream,
                                  size_t as_bytes);
typedef int (*lfa_launch_writev_t)(int dt, const struct lfa_iov_args *a, unsigned ntile,
                                   void *stream);
/* the fetch and compare list forms: the record says which pointer is which (lfa_iov.h) */
typedef lfa_launch_writev_t lfa_launch_fetchv_t;
typedef int (*lfa_launch_tree_t)(int dt, void *dst, const void *const *srcs, int nsrc,
                                 size_t cnt, void *stream, size_t as_bytes);
typedef int (*lfa_launch_treev_t)(int dt, const struct lfa_iov_args *a, int nsrc,
                                  unsigned ntile, void *stream);
typedef int (*lfa_launch_treeput_t)(int dt, void *const *dsts, int ndst, const void *const *srcs,
                                    int nsrc, size_t cnt, void *stream);
typedef int (*lfa_launch_oneshot_t)(int dt, const struct lfa_oneshot *a, void *stream, int ll);
typedef int (*lfa_launch_readwrite_t)(int dt, void *dst, const void *src, void *res, size_t cnt,
                                      void *stream, size_t as_bytes);
typedef int (*lfa_launch_swap_t)(int dt, void *dst, const void *src, const void *cmp, void *res,
                                 size_t cnt, void *stream, size_t as_bytes);

struct lfa_op_launch {
  lfa_launch_write_t write;         /* ops 0..9, 11 */
  lfa_launch_writev_t writev;       /* ops 0..9, 11 */
  lfa_launch_tree_t tree;           /* ops 0..9 */
  lfa_launch_treev_t treev;         /* ops 0..9 */
  lfa_launch_treeput_t treeput;     /* ops 0..9 */
  lfa_launch_oneshot_t oneshot;     /* ops 0..9 */
  lfa_launch_readwrite_t readwrite; /* ops 0..11 */
  lfa_launch_swap_t swap;           /* ops 12..18 */
  lfa_launch_fetchv_t readwritev;   /* ops 0..11 */
  lfa_launch_fetchv_t swapv;        /* ops 12..18 */
};

#endif /* LFA_LAUNCH_H */
