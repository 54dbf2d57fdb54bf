// The distance of one (x row, y row) pair as every nearest-neighbour kernel forms it (dudf_chamfer.hip, dudf_orient.hip), the
// finite test of a point the cloud kernels share (dudf_orient.hip, dudf_cloudprep.hip, dudf_bvh.hip) and the order-preserving code
// of a float (dudf_orient.hip, dudf_bvh.hip): device code only.  Internal: not installed, nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

constexpr float kFltMax = 3.402823466e+38f;
// false for an infinite or NaN coordinate
__device__ __forceinline__ bool finite3(float a, float b, float c) { return fabsf(a) <= kFltMax && fabsf(b) <= kFltMax && fabsf(c) <= kFltMax; }

// order-preserving code of a float: unsigned order of the codes is numeric order (atomicMin / atomicMax of bounds), and back
__device__ __forceinline__ unsigned float_code(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float code_float(unsigned c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7fffffffu) : ~c); }

// ONE sequence of roundings for every pair: the fused steps are written out and contraction is off, so the unrolled body, its
// remainder loop and any packed form the compiler picks give the same bits (a pair's distance must not depend on where in a tile it falls).
template <int NORM>
__device__ __forceinline__ float pair_distance(float ax, float ay, float az, const float4& q) {
#pragma clang fp contract(off)
    const float dx = ax - q.x, dy = ay - q.y, dz = az - q.z;
    if (NORM == 2) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    return (fabsf(dx) + fabsf(dy)) + fabsf(dz);
}
