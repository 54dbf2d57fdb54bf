// The ordered sum: the one rule by which a double sum over n rows comes out with the same bits on every call.
//   - groups = dudf_ordsum_groups(n) workgroups of kOrdSumBlock threads; thread t of group b adds rows b * 256 + t + k * groups * 256
//     in ascending k (the caller's loop);
//   - the workgroup adds its threads in a fixed halving tree (dudf_wg_tree): strides 128 .. 1;
//   - one workgroup adds the at most kOrdSumMaxGroups partials in index order (dudf_ordsum_finish).
// tests/ordered_sum_oracle.py restates it in numpy.  Additions only: nothing here depends on -ffp-contract.  Device code with one
// host helper.  Internal: not installed, nothing here is part of the C ABI.
#pragma once
#include "dudf_internal.h"

constexpr int kOrdSumBlock = 256;                // threads of a summing workgroup
constexpr int kOrdSumMaxGroups = 256;            // partials the single finishing workgroup adds in index order

// workgroups of a sum over n rows (at least one: an empty sum still has its partial)
inline int dudf_ordsum_groups(int64_t n) { return dudf_grid_for(n, kOrdSumBlock, kOrdSumMaxGroups); }

// what a tree does with an LDS array of one element per thread (DudfSumOf: K rows of them, ROW elements apart): s[i] takes s[j] in
template <class T, int K = 1, int ROW = 0> struct DudfSumOf {
    T* s;
    __device__ __forceinline__ void fold(int i, int j) const {
#pragma unroll
        for (int q = 0; q < K; ++q) s[q * ROW + i] += s[q * ROW + j];
    }
};
template <class T> struct DudfMaxOf { T* s; __device__ __forceinline__ void fold(int i, int j) const { const T o = s[j]; if (o > s[i]) s[i] = o; } };
template <class T> __device__ __forceinline__ DudfSumOf<T> dudf_sum_of(T* s) { return DudfSumOf<T>{s}; }
template <class T> __device__ __forceinline__ DudfMaxOf<T> dudf_max_of(T* s) { return DudfMaxOf<T>{s}; }

// A workgroup's BLOCK threads in a fixed tree; every array's result ends in its element 0.  All arrays ride the same barriers.  The
// first barrier closes the caller's stores of s[threadIdx.x].
template <int BLOCK, class... Arrays>
__device__ __forceinline__ void dudf_wg_tree(Arrays... arrays) {
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) (arrays.fold((int)threadIdx.x, (int)threadIdx.x + s), ...);
        __syncthreads();
    }
}

// A thread's K running sums -> the workgroup's K sums in partials[blockIdx.x * K + q].  Once per kernel: the LDS is the function's.
template <int BLOCK, int K>
__device__ __forceinline__ void dudf_ordsum_partial(const double (&v)[K], double* __restrict__ partials) {
    __shared__ double s[K][BLOCK];
#pragma unroll
    for (int q = 0; q < K; ++q) s[q][threadIdx.x] = v[q];
    dudf_wg_tree<BLOCK>(DudfSumOf<double, K, BLOCK>{&s[0][0]});
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) partials[blockIdx.x * K + q] = s[q][0];
    }
}

// The finishing workgroup (kOrdSumMaxGroups threads): partials[i * K + q], i < count <= kOrdSumMaxGroups, staged in LDS and added by
// thread 0 in index order.  out[] holds the K sums in thread 0 and zeros elsewhere; count == 0 gives zeros.
template <int K, class T>
__device__ __forceinline__ void dudf_ordsum_finish(const T* __restrict__ partials, int count, T (&out)[K]) {
    __shared__ T s[K][kOrdSumMaxGroups];
    if ((int)threadIdx.x < count) {
#pragma unroll
        for (int q = 0; q < K; ++q) s[q][threadIdx.x] = partials[K * threadIdx.x + q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) out[q] = 0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < count; ++i) {
#pragma unroll
            for (int q = 0; q < K; ++q) out[q] += s[q][i];
        }
    }
}
