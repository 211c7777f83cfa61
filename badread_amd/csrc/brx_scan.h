/*
 * brx_scan.h -- the tile scan: one inclusive prefix sum of 64-bit values over any number of elements, shared by the truth depth
 * (brx_depth.h), the window identities (brx_window.h) and the two device loaders (brx_pafin.h, brx_fastqin.h).  Each of them includes
 * this header itself.
 *
 * The contract, stated once:
 *   - Src is a functor copied into the kernels: `__device__ uint64_t operator()(uint64_t i) const` gives element i, i < n.  It is
 *     called twice per element (k_dp_reduce, k_dp_apply) and must return the same value both times; it may read neighbours of i.
 *   - dp_scan(st, src, n, sums, out): out[i] = the sum of src over [0, i].  `out` has n words and may not alias what src reads.
 *   - sums has n_tiles + 1 words, n_tiles = ceil(n / BRX_DEPTH_TILE) (include/brx.h: the tile is ABI, scratch sizes depend on it).
 *     After the call sums[t] = the sum before tile t and sums[n_tiles] = the total.  A caller that scans several lengths over one
 *     `sums` sizes it for the longest.
 *   - Three kernels per scan: k_dp_reduce (a sum per tile), k_dp_scan_sums (one workgroup over the tile sums), k_dp_apply (the tile's
 *     own scan on top of its sum).  Order between workgroups comes from kernel boundaries alone: no workgroup waits for another and
 *     global memory takes no atomics.  Callers scan n >= 1: a grid of no workgroups is not a launch.
 */
#ifndef BRX_SCAN_H
#define BRX_SCAN_H

#include "brx_kernels.h"

#define BRX_DP_THREADS 256u
#define BRX_DP_ITEMS (BRX_DEPTH_TILE / BRX_DP_THREADS)

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v) {
    const int lane = lane_id();
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, dd, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), dd, 64);
        if (lane >= dd) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
/* Inclusive scan of v over the workgroup's threads in thread order; *total = the workgroup's sum.  lds: a word per wave.  Every thread
   calls it. */
__device__ __forceinline__ uint64_t dp_block_scan(uint64_t v, uint64_t *lds, uint64_t *total) {
    const uint32_t w = threadIdx.x >> 6;
    const uint64_t inc = wave_incl_scan_u64(v);
    __syncthreads();                                   /* the words of the call before have been read */
    if (lane_id() == 63) lds[w] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_THREADS / 64u; ++x) { const uint64_t s = lds[x]; if (x < w) base += s; tot += s; }
    *total = tot;
    return base + inc;
}

/* sums[tile] = the sum of src over the tile; a thread takes BRX_DP_ITEMS consecutive elements */
template <class Src>
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_reduce(Src src, uint64_t n, uint64_t *sums) {
    __shared__ uint64_t lds[BRX_DP_THREADS / 64u];
    const uint64_t i0 = (uint64_t)blockIdx.x * BRX_DEPTH_TILE + (uint64_t)threadIdx.x * BRX_DP_ITEMS;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) if (i0 + x < n) v += src(i0 + x);
    uint64_t tot;
    dp_block_scan(v, lds, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
/* the tile sums to what lies before each tile, in place; sums[n_tiles] = the total.  One workgroup. */
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_scan_sums(uint64_t *sums, uint32_t n_tiles) {
    __shared__ uint64_t lds[BRX_DP_THREADS / 64u];
    uint64_t run = 0;
    for (uint32_t b = 0; b < n_tiles; b += BRX_DP_THREADS) {
        const uint32_t i = b + threadIdx.x;
        const uint64_t v = i < n_tiles ? sums[i] : 0u;
        uint64_t tot;
        const uint64_t inc = dp_block_scan(v, lds, &tot);
        if (i < n_tiles) sums[i] = run + inc - v;
        run += tot;
    }
    if (threadIdx.x == 0) sums[n_tiles] = run;
}
/* out[i] = the sum of src over [0, i] */
template <class Src>
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_apply(Src src, uint64_t n, const uint64_t *sums, uint64_t *out) {
    __shared__ uint64_t lds[BRX_DP_THREADS / 64u];
    const uint64_t i0 = (uint64_t)blockIdx.x * BRX_DEPTH_TILE + (uint64_t)threadIdx.x * BRX_DP_ITEMS;
    uint64_t val[BRX_DP_ITEMS], v = 0;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) { val[x] = i0 + x < n ? src(i0 + x) : 0u; v += val[x]; }
    uint64_t tot;
    uint64_t run = sums[blockIdx.x] + dp_block_scan(v, lds, &tot) - v;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) { run += val[x]; if (i0 + x < n) out[i0 + x] = run; }
}

/* the plainest source: a table of 32-bit counts */
struct DpSrcTable { const uint32_t *t; __device__ uint64_t operator()(uint64_t i) const { return t[i]; } };

/* one inclusive scan: out[i] = the sum of src over [0, i] */
template <class Src> static void dp_scan(hipStream_t st, Src src, uint64_t n, uint64_t *sums, uint64_t *out) {
    const uint32_t nt = (uint32_t)((n + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    hipLaunchKernelGGL((k_dp_reduce<Src>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, src, n, sums);
    hipLaunchKernelGGL(k_dp_scan_sums, dim3(1), dim3(BRX_DP_THREADS), 0, st, sums, nt);
    hipLaunchKernelGGL((k_dp_apply<Src>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, src, n, (const uint64_t *)sums, out);
}

#endif /* BRX_SCAN_H */
