// lfa_tune_forms.hpp — forms of the product kernels' templates that only the
// tuning library (liblfa_tune.so: lfa_tune.hip, lfa_tune_b.hip) instantiates:
// the register-staged references the product bodies were measured against and
// the tree variants bench.py --tune-tree times at every fan-in.  No product
// object includes this file.
#pragma once

#include "lfa_kernels.hpp"

namespace lfa {

// ---------------------------------------------------------------------------
// binary combine, register staged
// ---------------------------------------------------------------------------
// Chunked: workgroup b owns vectors [b·kBlock·U, (b+1)·kBlock·U); step u of
// thread t touches base + u·kBlock + t, i.e. each wave-instruction reads 1 KiB
// of consecutive bytes.  All 2·U loads issue before the first op.
template <int OP, typename T, int U, bool NTL, bool NTS>
__global__ __launch_bounds__(kBlock) void combine_vec(
    u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, size_t nvec) {
  const size_t base = (size_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  if (base + (size_t)(U - 1) * kBlock < nvec) {  // full chunk: no guards
    u32x4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = ld<NTL>(dst + base + u * kBlock);
#pragma unroll
    for (int u = 0; u < U; u++) b[u] = ld<NTL>(src + base + u * kBlock);
#pragma unroll
    for (int u = 0; u < U; u++)
      st<NTS>(dst + base + u * kBlock, apply_vec<OP, T>(a[u], b[u]));
  } else {
#pragma unroll
    for (int u = 0; u < U; u++) {
      size_t i = base + (size_t)u * kBlock;
      if (i < nvec)
        st<NTS>(dst + i, apply_vec<OP, T>(ld<NTL>(dst + i), ld<NTL>(src + i)));
    }
  }
}

// Grid-stride variant: a fixed grid of G workgroups walks the buffer; each
// thread holds U vectors spaced kBlock apart.
template <int OP, typename T, int U, bool NTL, bool NTS>
__global__ __launch_bounds__(kBlock) void combine_vec_gs(
    u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, size_t nvec) {
  const size_t step = (size_t)gridDim.x * kBlock * U;
  size_t base = (size_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  for (; base + (size_t)(U - 1) * kBlock < nvec; base += step) {
    u32x4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = ld<NTL>(dst + base + u * kBlock);
#pragma unroll
    for (int u = 0; u < U; u++) b[u] = ld<NTL>(src + base + u * kBlock);
#pragma unroll
    for (int u = 0; u < U; u++)
      st<NTS>(dst + base + u * kBlock, apply_vec<OP, T>(a[u], b[u]));
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    size_t i = base + (size_t)u * kBlock;
    if (i < nvec)
      st<NTS>(dst + i, apply_vec<OP, T>(ld<NTL>(dst + i), ld<NTL>(src + i)));
  }
}

// ---------------------------------------------------------------------------
// fetch / compare, register staged (round 1): 2 vectors per lane
// ---------------------------------------------------------------------------
constexpr int kFetchUnroll = 2;

template <typename F>
__global__ __launch_bounds__(kBlock) void fetch_vec(F f, size_t nvec) {
  const size_t base = (size_t)blockIdx.x * (kBlock * kFetchUnroll) + threadIdx.x;
#pragma unroll
  for (int u = 0; u < kFetchUnroll; u++) {
    size_t i = base + (size_t)u * kBlock;
    if (i < nvec) f.vec(i);
  }
}

// ---------------------------------------------------------------------------
// N-input tree
// ---------------------------------------------------------------------------
// Grid-stride form (tuning reference): plain loads, one vector per lane.
template <int OP, typename T, int NLEAF>
__global__ __launch_bounds__(kBlock) void reduce_tree_vec(TreeArgs a,
                                                          u32x4 *dst,
                                                          size_t nvec) {
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  size_t stride = (size_t)gridDim.x * kBlock;
  for (; i < nvec; i += stride)
    st<true>(dst + i, tree_eval<OP, T, u32x4, NLEAF>(a, i));
}

// Wave-contiguous register form: wave w of workgroup b owns U consecutive KiB
// of every input (longer DRAM bursts per input stream than the chunked form).
template <int OP, typename T, int NLEAF, int U>
__global__ __launch_bounds__(kBlock) void reduce_tree_wave(TreeArgs a,
                                                           u32x4 *dst,
                                                           size_t nvec) {
  const unsigned w = threadIdx.x / 64, l = threadIdx.x % 64;
  const size_t base = (size_t)blockIdx.x * (kBlock * U) + (size_t)w * 64 * U + l;
#pragma unroll
  for (int u = 0; u < U; u++) {
    size_t i = base + (size_t)u * 64;
    if (i < nvec)
      st<true>(dst + i, tree_eval_with<OP, T, u32x4, NLEAF>(a, [&](int k) {
                 return ld<true>((const u32x4 *)a.in[k] + i);
               }));
  }
}

// Tapered chunk form (variant 12, the combine's tapered tail applied to the
// tree): workgroups [0, head) take U = 2 vectors per lane up to vector
// `split`, the rest — dispatched last — one vector per lane, so the waves that
// end the launch are shorter.  Write-through stores (the chunk form's sc1).
template <int OP, typename T, int NLEAF, int U>
__device__ __forceinline__ void tree_chunk_at(const TreeArgs &a, u32x4 *dst, size_t nvec,
                                              size_t wg0) {
#pragma unroll
  for (int u = 0; u < U; u++) {
    const size_t i = wg0 + (size_t)u * kBlock + threadIdx.x;
    if (i < nvec) {
      u32x4 v = tree_eval_with<OP, T, u32x4, NLEAF>(
          a, [&](int k) { return ld<true>((const u32x4 *)a.in[k] + i); });
      const size_t wb = wg0 + (size_t)u * kBlock + (size_t)wave_id() * 64;
      __builtin_amdgcn_raw_buffer_store_b128(
          v, __builtin_amdgcn_make_buffer_rsrc(dst + wb, 0, 64 * 16, 0x00020000),
          (threadIdx.x % 64) * 16, 0, kStoreSc1);
    }
  }
}

template <int OP, typename T, int NLEAF>
__global__ __launch_bounds__(kBlock) void reduce_tree_taper(TreeArgs a, u32x4 *dst, size_t nvec,
                                                            size_t split, unsigned head) {
  const unsigned b = blockIdx.x;
  if (b < head)
    tree_chunk_at<OP, T, NLEAF, 2>(a, dst, split, (size_t)b * (kBlock * 2));
  else
    tree_chunk_at<OP, T, NLEAF, 1>(a, dst, nvec, split + (size_t)(b - head) * kBlock);
}

// The tree vector bodies of launch_tree_body (lfa_k_launch.hpp) at every
// fan-in, not only where the product selects them (1, 2, 3, 25), and the
// variants it never selects.  False: not one of these, the caller falls
// through to the product's launcher.
template <int OP, typename T, int NLEAF>
static bool launch_tree_tune_form(const TreeArgs &b, int nsrc, u32x4 *dst, size_t nvec,
                                  hipStream_t s, int variant) {
  auto chunk = [&](auto kern, int u, unsigned lds) {
    hipLaunchKernelGGL(kern, dim3(grid_for(nvec, (size_t)kBlock * u, 0x7fffffffu)),
                       dim3(kBlock), lds, s, b, dst, nvec);
  };
  auto put = [&](auto kern, int u, unsigned lds) {
    PutArgs pa;
    pa.t = b;
    memset(pa.out, 0, sizeof(pa.out));
    pa.out[0] = dst;
    pa.nout = 1;
    hipLaunchKernelGGL(kern, dim3(grid_for(nvec, (size_t)kBlock * u, 0x7fffffffu)),
                       dim3(kBlock), lds, s, pa, nvec);
  };
  // round 5: dynamic LDS the bodies never touch caps the workgroups per CU
  constexpr unsigned kCap[5] = {41u << 10, 54u << 10, 81u << 10, 0u, 54u << 10};
  switch (variant) {
    case 1: chunk(reduce_tree_chunk<OP, T, NLEAF, 1>, 1, 0); return true;
    case 2: chunk(reduce_tree_chunk<OP, T, NLEAF, 2>, 2, 0); return true;
    case 3: launch_tree_lds<OP, T, NLEAF, kLdsWaves, 1>(b, nsrc, dst, nvec, s); return true;
    case 12: {
      // the last 1/8 of the vectors one per lane (reduce_tree_taper)
      const lfa_taper tp = lfa_split_taper(nvec, 8, (size_t)kBlock * 2, kBlock);
      hipLaunchKernelGGL((reduce_tree_taper<OP, T, NLEAF>), dim3(tp.nhead + tp.ntail),
                         dim3(kBlock), 0, s, b, dst, nvec, tp.split, tp.nhead);
      return true;
    }
    // round 5: the write-through chunk form at capped occupancy and at 4
    // vectors per lane
    case 20: case 21: case 22:
      chunk(reduce_tree_chunk<OP, T, NLEAF, 2, kStoreSc1>, 2, kCap[variant - 20]);
      return true;
    case 23: case 24:
      chunk(reduce_tree_chunk<OP, T, NLEAF, 4, kStoreSc1>, 4, kCap[variant - 20]);
      return true;
    // round 5: the P2P push kernel's body with one output (tile-sized buffer
    // descriptors, system-scope nt loads, write-through stores) at 4 KiB per
    // wave per input (25; 26 at <= 3 workgroups per CU) and at 2 KiB (27; 28
    // at <= 3 workgroups per CU)
    case 25: case 26:
      put(reduce_tree_put<OP, T, NLEAF, 4>, 4, variant == 26 ? (41u << 10) : 0u);
      return true;
    case 27: case 28:
      put(reduce_tree_put<OP, T, NLEAF, 2>, 2, variant == 28 ? (41u << 10) : 0u);
      return true;
    default: return false;
  }
}

}  // namespace lfa
