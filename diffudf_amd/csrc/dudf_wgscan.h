// Index and compaction toolkit of the extraction units (point cloud and render gather, CAP-UDF cells, Lewiner marching cubes): device
// code only.  Internal: not installed, nothing here is part of the C ABI.
//   dudf_wg_rank, dudf_wg_scan: ballot rank and exclusive scan over a workgroup of DUDF_WG = 256 threads (four waves);
//   dudf_wg_item, dudf_wg_add_total: the thread's item, and a workgroup total added to a 64-bit counter;
//   dudf_scan_totals_kernel<K>: exclusive scan of per-workgroup totals, one 1024-thread workgroup
//   dudf_wg_scan64, dudf_scan_totals64_kernel: the same two over 64-bit unsigned integers (the surface sampler's cumulative weights)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int DUDF_WG = 256;                             // threads of the workgroups below: four waves of 64

// Flagged threads before this one, in thread order; *total = flagged threads of the workgroup.  wave_tot: DUDF_WG / 64 words of
// LDS.  Both barriers are the helper's own: it can be called again at once (a grid-stride loop over tiles) with the same words.
__device__ __forceinline__ unsigned dudf_wg_rank(bool flag, unsigned* wave_tot, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wave_tot[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned before = (unsigned)__popcll(b & ((1ull << lane) - 1ull)), sum = 0;
    for (int q = 0; q < wave; ++q) before += wave_tot[q];            // a wave-uniform trip count: no per-lane selects
    for (int q = 0; q < DUDF_WG / 64; ++q) sum += wave_tot[q];
    __syncthreads();
    *total = sum;
    return before;
}

// The item of this thread in a grid of DUDF_WG-thread workgroups, one thread per item.
__device__ __forceinline__ int64_t dudf_wg_item() { return (int64_t)blockIdx.x * DUDF_WG + threadIdx.x; }
// Thread 0 adds the workgroup's total (the *total of a rank or a scan) to a 64-bit counter: one atomic per workgroup that counted anything.
__device__ __forceinline__ void dudf_wg_add_total(unsigned long long* ctr, unsigned total) {
    if (threadIdx.x == 0 && total) atomicAdd(ctr, (unsigned long long)total);
}

// Exclusive scan of a small count over the workgroup's threads (thread order); *total = the sum.  wave_tot as above; the leading
// barrier lets the words be reused straight after any other use of them.
__device__ __forceinline__ unsigned dudf_wg_scan(unsigned w, unsigned* wave_tot, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    unsigned before = 0, sum = 0;
    for (int q = 0; q < wave; ++q) before += wave_tot[q];            // a wave-uniform trip count: no per-lane selects
    for (int q = 0; q < DUDF_WG / 64; ++q) sum += wave_tot[q];
    *total = sum;
    return before + inc - w;
}

// dudf_wg_scan over 64-bit unsigned integers: wave_tot is DUDF_WG / 64 64-bit words.  Integer sums wrap, they do not round: the
// result is the same in any order.
__device__ __forceinline__ unsigned long long dudf_wg_scan64(unsigned long long w, unsigned long long* wave_tot,
                                                             unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, sum = 0;
    for (int q = 0; q < wave; ++q) before += wave_tot[q];            // a wave-uniform trip count: no per-lane selects
    for (int q = 0; q < DUDF_WG / 64; ++q) sum += wave_tot[q];
    *total = sum;
    return before + inc - w;
}

// Exclusive scan of per-workgroup totals: blk [nblocks][K] uint32 -> off [nblocks][K] int64, the K grand totals -> out_counts.
// One workgroup of 1024 threads (static LDS K * 8 KiB); thread t sums blocks [t * chunk, (t + 1) * chunk) clamped to nblocks —
// an empty range for the upper threads of a short array —, the partial sums are scanned, and the thread writes its blocks' offsets.
// static: an instantiation stays inside the unit that launches it, like the kernels beside it.
template <int K>
static __global__ __launch_bounds__(1024) void dudf_scan_totals_kernel(const uint32_t* __restrict__ blk, int64_t* __restrict__ off,
                                                                       int64_t nblocks, int64_t* __restrict__ out_counts) {
    __shared__ int64_t s[K][1024];
    const int t = threadIdx.x;
    const int64_t chunk = (nblocks + 1023) / 1024;
    const int64_t b0 = (int64_t)t * chunk < nblocks ? (int64_t)t * chunk : nblocks, b1 = (b0 + chunk < nblocks) ? b0 + chunk : nblocks;
    int64_t sum[K] = {};
    for (int64_t b = b0; b < b1; ++b)
        for (int q = 0; q < K; ++q) sum[q] += blk[b * K + q];
    for (int q = 0; q < K; ++q) s[q][t] = sum[q];
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                  // inclusive Hillis-Steele over the 1024 partial sums
        int64_t add[K] = {};
        if (t >= d) for (int q = 0; q < K; ++q) add[q] = s[q][t - d];
        __syncthreads();
        for (int q = 0; q < K; ++q) s[q][t] += add[q];
        __syncthreads();
    }
    int64_t run[K];
    for (int q = 0; q < K; ++q) run[q] = s[q][t] - sum[q];
    for (int64_t b = b0; b < b1; ++b)
        for (int q = 0; q < K; ++q) { off[b * K + q] = run[q]; run[q] += blk[b * K + q]; }
    if (t == 1023) for (int q = 0; q < K; ++q) out_counts[q] = s[q][1023];
}

// dudf_scan_totals_kernel<1> over 64-bit totals: blk [nblocks] uint64 -> off [nblocks] uint64 (exclusive), the grand total ->
// *out_total.  The same one workgroup of 1024 threads and the same chunking.
static __global__ __launch_bounds__(1024) void dudf_scan_totals64_kernel(const uint64_t* __restrict__ blk, uint64_t* __restrict__ off,
                                                                         int64_t nblocks, uint64_t* __restrict__ out_total) {
    __shared__ uint64_t s[1024];
    const int t = threadIdx.x;
    const int64_t chunk = (nblocks + 1023) / 1024;
    const int64_t b0 = (int64_t)t * chunk < nblocks ? (int64_t)t * chunk : nblocks, b1 = (b0 + chunk < nblocks) ? b0 + chunk : nblocks;
    uint64_t sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += blk[b];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                  // inclusive Hillis-Steele over the 1024 partial sums
        const uint64_t add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    uint64_t run = s[t] - sum;
    for (int64_t b = b0; b < b1; ++b) { off[b] = run; run += blk[b]; }
    if (t == 1023) *out_total = s[1023];
}
