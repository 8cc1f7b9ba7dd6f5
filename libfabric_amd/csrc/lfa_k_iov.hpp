// lfa_k_iov.hpp — the list (fi_ioc) forms: every segment of a call combined
// in ONE launch (lfa_atomic_writev_async, lfa_reduce_treev_async,
// lfa_atomic_readwritev_async, lfa_atomic_swapv_async).
// Part of lfa_kernels.hpp; included by it after the launchers.  Not included
// on its own.  Table layout and tiling: lfa_iov.h.
//
// Workgroup b owns tile b of the call: it finds its (segment, tile) in the
// prefix table — a binary search over wave-uniform words, or no search at all
// when every segment is a single tile — reads the segment's record and runs
// the element semantics of lfa_ops.hpp on its 16 KiB of dst, on the path the
// segment's own alignment permits:
//   vector   dst and the inputs 16-byte co-aligned: the binary form runs the
//            product's LDS-DMA tile (lds_tile, 4 KiB per wave per operand,
//            write-through stores), the tree form four nt-loaded vectors per
//            lane through tree_eval_with; the elements before dst's first
//            16-byte boundary are done once by tile 0 and those after the
//            last whole vector once by the tile that holds them (one element
//            loop per kernel serves heads, tails and the paths below)
//   element  aligned to the element, not co-aligned: one element per lane
//   bytes    some operand not aligned to the element: byte-wise moves
// so a call's result is bit for bit that of one lfa_atomic_write_async /
// lfa_reduce_tree_async / lfa_atomic_readwrite_async / lfa_atomic_swap_async
// per segment.  The fetch and compare forms (fetch_iov) run the fetch
// family's LDS-DMA tile, fetch_tile, on the vector path.
#pragma once

#include "lfa_iov.h"

namespace lfa {

typedef lfa_iov_args IovArgs;

struct IovTreeArgs {
  IovArgs a;
  signed char hi[kMaxLeaf];  // TreeArgs' leaf pairing, the same for every segment
  signed char lo[kMaxLeaf];
};

constexpr unsigned kIovTileVecs = LFA_IOV_TILE / 16;
// The fused list form is instantiated up to 8 leaves (2..15 inputs), the
// fan-ins of a node's GPUs; a wider tree is one lfa_reduce_tree_async per
// segment (lfa_iov.cpp), which keeps a fifth kernel family of 16- and
// 32-leaf bodies out of liblfa.so.
constexpr int kIovMaxLeaf = LFA_IOV_TREE_LEAVES;
static_assert(kIovTileVecs == kLdsWaves * 64 * kUnroll, "a tile is one workgroup of lds_tile");

__device__ __forceinline__ uint64_t iov_word(const IovArgs &a, uint32_t i) {
  return a.tab ? a.tab[i] : a.inl[i];
}

__device__ __forceinline__ uint32_t iov_first_tile(const IovArgs &a, uint32_t s) {
  const uint64_t w = iov_word(a, s >> 1);
  return (uint32_t)(s & 1 ? w >> 32 : w);
}

// This workgroup's segment record (its first word's index) and tile within
// the segment.  Everything here is the same on every lane: scalar.
__device__ __forceinline__ uint32_t iov_find(const IovArgs &a, uint32_t &tile) {
  const uint32_t b = blockIdx.x;
  uint32_t seg = b;
  tile = 0;
  if (!a.direct) {
    uint32_t lo = 0, hi = a.nseg;  // first_tile[lo] <= b < first_tile[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (iov_first_tile(a, mid) <= b) lo = mid;
      else hi = mid;
    }
    seg = lo;
    tile = b - iov_first_tile(a, lo);
  }
  seg = __builtin_amdgcn_readfirstlane(seg);
  tile = __builtin_amdgcn_readfirstlane(tile);
  return (uint32_t)lfa_iov_prefix_words(a.nseg) + seg * (LFA_IOV_IN + a.nin);
}

// ---------------------------------------------------------------------------
// dst[s][i] = dst[s][i] OP src[s][i], every segment s in one launch
// ---------------------------------------------------------------------------
template <int OP, typename T>
__global__ __launch_bounds__(kLdsWaves * 64) void combine_iov(IovArgs a) {
  __shared__ u32x4 lds[2][kLdsWaves][kUnroll][64];
  constexpr size_t E = sizeof(T), TE = LFA_IOV_TILE / E;
  uint32_t tile;
  const uint32_t r = iov_find(a, tile);
  char *dst = (char *)iov_word(a, r + LFA_IOV_DST);
  const size_t cnt = iov_word(a, r + LFA_IOV_COUNT);
  const char *src = (const char *)iov_word(a, r + LFA_IOV_IN);
  const uintptr_t pd = (uintptr_t)dst, ps = (uintptr_t)src;
  const unsigned t = threadIdx.x;
  if (pd % E || ps % E) {
    const size_t i0 = (size_t)tile * TE, i1 = cnt - i0 < TE ? cnt : i0 + TE;
    for (size_t i = i0 + t; i < i1; i += kLdsWaves * 64)
      st_bytes<T>(dst, i, apply<OP, T>(ld_bytes<T>(dst, i), ld_bytes<T>(src, i)));
    return;
  }
  T *de = (T *)dst;
  const T *se = (const T *)src;
  // Element work of this tile: [0, n0) and [off1, off1 + n1), one call site.
  // Tile 0 always owns the head, the elements before dst's first 16-byte
  // boundary.
  const size_t head = lfa_split_head(pd, cnt, E), n0 = tile == 0 ? head : 0;
  size_t off1, n1;
  if ((pd ^ ps) % 16 == 0) {
    const size_t nvec = (cnt - head) * E / 16;
    const unsigned w = wave_id<true>(), l = t % 64;
    lds_tile<OP, T, kUnroll, kUnroll, kStoreSc1>(
        (u32x4 *)(dst + head * E), (const u32x4 *)(src + head * E), nvec,
        (size_t)tile * kIovTileVecs + (size_t)w * 64 * kUnroll, lds, w, l);
    // the elements after the last whole vector: once, by the tile they lie in
    off1 = head + nvec * (16 / E);
    n1 = tile == nvec / kIovTileVecs ? cnt - off1 : 0;
  } else {
    const size_t rest = cnt - head, i0 = (size_t)tile * TE;
    off1 = head + i0;
    n1 = rest - i0 < TE ? rest - i0 : TE;
  }
  for (size_t i = t; i < n0 + n1; i += kLdsWaves * 64) {
    const size_t k = i < n0 ? i : off1 + (i - n0);
    de[k] = apply<OP, T>(de[k], se[k]);
  }
}

// ---------------------------------------------------------------------------
// dst[s] = prov/coll's tree of in[s][0 .. nin), every segment s in one launch
// ---------------------------------------------------------------------------
template <int OP, typename T, int NLEAF>
__global__ __launch_bounds__(kBlock) void reduce_iov(IovTreeArgs ta) {
  constexpr size_t E = sizeof(T), TE = LFA_IOV_TILE / E;
  const IovArgs &a = ta.a;
  uint32_t tile;
  const uint32_t r = iov_find(a, tile);
  char *dst = (char *)iov_word(a, r + LFA_IOV_DST);
  const size_t cnt = iov_word(a, r + LFA_IOV_COUNT);
  auto in = [&](int k) { return (const char *)iov_word(a, r + LFA_IOV_IN + k); };
  const uintptr_t pd = (uintptr_t)dst;
  uintptr_t any = pd, mis = 0;
  for (uint32_t k = 0; k < a.nin; k++) {  // wave-uniform
    const uintptr_t p = (uintptr_t)in(k);
    any |= p;
    mis |= p ^ pd;
  }
  const unsigned t = threadIdx.x;
  // Element work of this tile: [0, n0) and [off1, off1 + n1), one call site;
  // `bytes`: some operand is not aligned to the element and all move byte-wise.
  const bool bytes = any % E != 0;
  const size_t head = bytes ? 0 : lfa_split_head(pd, cnt, E), n0 = tile == 0 ? head : 0;
  size_t off1, n1;
  if (!bytes && mis % 16 == 0) {
    const size_t nvec = (cnt - head) * E / 16, hb = head * E;
    u32x4 *dv = (u32x4 *)(dst + hb);
#pragma unroll 2
    for (int u = 0; u < kUnroll; u++) {
      const size_t i = (size_t)tile * kIovTileVecs + (size_t)u * kBlock + t;
      if (i < nvec)
        st<true>(dv + i, tree_eval_with<OP, T, u32x4, NLEAF>(ta, [&](int k) {
                   return ld<true>((const u32x4 *)(in(k) + hb) + i);
                 }));
    }
    off1 = head + nvec * (16 / E);
    n1 = tile == nvec / kIovTileVecs ? cnt - off1 : 0;
  } else {
    const size_t rest = cnt - head, i0 = (size_t)tile * TE;
    off1 = head + i0;
    n1 = rest - i0 < TE ? rest - i0 : TE;
  }
  for (size_t i = t; i < n0 + n1; i += kBlock) {
    const size_t k = i < n0 ? i : off1 + (i - n0);
    const T v = tree_eval_with<OP, T, T, NLEAF>(ta, [&](int s) {
      return bytes ? ld_bytes<T>(in(s), k) : ((const T *)in(s))[k];
    });
    if (bytes) st_bytes<T>(dst, k, v);
    else ((T *)dst)[k] = v;
  }
}

// ---------------------------------------------------------------------------
// res[s][i] = dst[s][i], then dst[s][i] is updated: the fetch (readwritev) and
// compare (swapv) tables, every segment s in one launch
// ---------------------------------------------------------------------------
// A segment's functor (lfa_k_fetch.hpp) from its record; the vector pointers
// start `hb` bytes in, after the head.  ATOMIC_READ's record carries dst in
// the src word (lfa_iov.cpp), which RwF<OP_READ> never dereferences.
template <int OP, typename T, bool A>
__device__ __forceinline__ void iov_functor(RwF<OP, T, A> &f, const IovArgs &a, uint32_t r,
                                            size_t hb) {
  static_assert(RwF<OP, T, A>::kIn <= LFA_IOV_RW_NIN, "src and res travel in the record");
  char *d = (char *)iov_word(a, r + LFA_IOV_DST);
  const char *s = (const char *)iov_word(a, r + LFA_IOV_RW_SRC);
  char *res = (char *)iov_word(a, r + LFA_IOV_RW_RES);
  f = RwF<OP, T, A>{d, s, res, (u32x4 *)(d + hb), (const u32x4 *)(s + hb), (u32x4 *)(res + hb)};
}

template <int OP, typename T, bool A>
__device__ __forceinline__ void iov_functor(SwapF<OP, T, A> &f, const IovArgs &a, uint32_t r,
                                            size_t hb) {
  static_assert(SwapF<OP, T, A>::kIn == LFA_IOV_SWAP_NIN, "src, cmp and res travel in the record");
  char *d = (char *)iov_word(a, r + LFA_IOV_DST);
  const char *s = (const char *)iov_word(a, r + LFA_IOV_SWAP_SRC);
  const char *c = (const char *)iov_word(a, r + LFA_IOV_SWAP_CMP);
  char *res = (char *)iov_word(a, r + LFA_IOV_SWAP_RES);
  f = SwapF<OP, T, A>{d,
                      s,
                      c,
                      res,
                      (u32x4 *)(d + hb),
                      (const u32x4 *)(s + hb),
                      (const u32x4 *)(c + hb),
                      (u32x4 *)(res + hb)};
}

// FA / FB: one functor family's element-aligned and byte-wise members (RwF or
// SwapF of one (OP, T)).  The path is launch_fetch's, decided here per segment
// over ALL of the record's pointers (dst, src, [cmp,] res); whole-vector tiles
// run fetch_tile as the contiguous launcher does below kSc1Bytes (4 KiB per
// input per wave, write-through stores, the two-input body drained); its
// buffer resources are cut from the functor's pointers, so from the record.
template <typename FA, typename FB, typename T>
__global__ __launch_bounds__(kLdsWaves * 64) void fetch_iov(IovArgs a) {
  __shared__ u32x4 lds[FA::kIn][kLdsWaves][kUnroll][64];
  constexpr size_t E = sizeof(T), TE = LFA_IOV_TILE / E;
  uint32_t tile;
  const uint32_t r = iov_find(a, tile);
  const uintptr_t pd = (uintptr_t)iov_word(a, r + LFA_IOV_DST);
  const size_t cnt = iov_word(a, r + LFA_IOV_COUNT);
  uintptr_t any = pd, mis = 0;
  for (uint32_t k = 0; k < a.nin; k++) {  // wave-uniform
    const uintptr_t p = (uintptr_t)iov_word(a, r + LFA_IOV_IN + k);
    any |= p;
    mis |= p ^ pd;
  }
  const unsigned t = threadIdx.x;
  // Element work of this tile: [0, n0) and [off1, off1 + n1), one call site;
  // `bytes`: some operand is not aligned to the element and all move byte-wise.
  const bool bytes = any % E != 0;
  const size_t head = bytes ? 0 : lfa_split_head(pd, cnt, E), n0 = tile == 0 ? head : 0;
  FA fa;
  FB fb;
  iov_functor(fa, a, r, head * E);
  iov_functor(fb, a, r, 0);
  size_t off1, n1;
  if (!bytes && mis % 16 == 0) {
    const size_t nvec = (cnt - head) * E / 16;
    const unsigned w = wave_id<true>(), l = t % 64;
    fetch_tile<kUnroll, kUnroll, kStoreSc1, FA, FA::kIn == 2>(
        fa, nvec, (size_t)tile * kIovTileVecs + (size_t)w * 64 * kUnroll, lds, w, l);
    // the elements after the last whole vector: once, by the tile they lie in
    off1 = head + nvec * (16 / E);
    n1 = tile == nvec / kIovTileVecs ? cnt - off1 : 0;
  } else {
    const size_t rest = cnt - head, i0 = (size_t)tile * TE;
    off1 = head + i0;
    n1 = rest - i0 < TE ? rest - i0 : TE;
  }
  for (size_t i = t; i < n0 + n1; i += kLdsWaves * 64) {
    const size_t k = i < n0 ? i : off1 + (i - n0);
    if (E > 1 && bytes) fb.elem(k);
    else fa.elem(k);
  }
}

// ---------------------------------------------------------------------------
// launchers: the table is built and validated by lfa_iov.cpp
// ---------------------------------------------------------------------------
static_assert(kBlock == kLdsWaves * 64, "one workgroup shape for both forms");

template <int OP, typename T>
static int launch_readwritev(const IovArgs &a, unsigned ntile, hipStream_t s) {
  if constexpr (!rw_supported<OP, T>()) {
    return -LFA_EOPNOTSUPP;
  } else {
    hipLaunchKernelGGL((fetch_iov<RwF<OP, T, true>, RwF<OP, T, false>, T>), dim3(ntile),
                       dim3(kBlock), 0, s, a);
    return launch_rc();
  }
}

template <int OP, typename T>
static int launch_swapv(const IovArgs &a, unsigned ntile, hipStream_t s) {
  if constexpr (!swap_supported<OP, T>()) {
    return -LFA_EOPNOTSUPP;
  } else {
    hipLaunchKernelGGL((fetch_iov<SwapF<OP, T, true>, SwapF<OP, T, false>, T>), dim3(ntile),
                       dim3(kBlock), 0, s, a);
    return launch_rc();
  }
}

template <int OP, typename T>
static int launch_writev(const IovArgs &a, unsigned ntile, hipStream_t s) {
  if constexpr (!supported<OP, T>()) {
    return -LFA_EOPNOTSUPP;
  } else {
    hipLaunchKernelGGL((combine_iov<OP, T>), dim3(ntile), dim3(kBlock), 0, s, a);
    return launch_rc();
  }
}

template <int OP, typename T>
static int launch_treev(const IovArgs &a, int nsrc, unsigned ntile, hipStream_t s) {
  if constexpr (!supported<OP, T>()) {
    return -LFA_EOPNOTSUPP;
  } else {
    if (nsrc < 2 || nsrc >= 2 * kIovMaxLeaf) return -LFA_EINVAL;
    IovTreeArgs ta;
    TreeArgs pairing;
    const void *none[kMaxLeaf] = {};
    const int pof2 = tree_leaves(pairing, none, nsrc);
    ta.a = a;
    memcpy(ta.hi, pairing.hi, sizeof(ta.hi));
    memcpy(ta.lo, pairing.lo, sizeof(ta.lo));
    const dim3 grid(ntile), block(kBlock);
    switch (pof2) {
      case 2: hipLaunchKernelGGL((reduce_iov<OP, T, 2>), grid, block, 0, s, ta); break;
      case 4: hipLaunchKernelGGL((reduce_iov<OP, T, 4>), grid, block, 0, s, ta); break;
      case 8: hipLaunchKernelGGL((reduce_iov<OP, T, 8>), grid, block, 0, s, ta); break;
      default: return -LFA_EINVAL;
    }
    return launch_rc();
  }
}

}  // namespace lfa
