// Builds the index of dudf_bvh.h over triangles (dudf_mesh_*) or points (dudf_cloud_*): one set of kernels and one driver over a
// primitive trait.  Kernels and their C entry points (include/dudf_hip.h).
#include "dudf_bvh.h"

namespace {

constexpr int kGridCap = 8192;                   // workgroups of the build launches; the kernels stride over the rest

// What the build needs to know about a primitive: its floats in the caller's array, its Morton key, its sorted copy.
struct TriPrim {                                 // a triangle: three vertices
    static constexpr int kFloats = 9;
    using Layout = GwMeshLayout;
    static Layout carve(const void* index, int64_t n) { return gw_carve_mesh(index, n); }
    static __device__ __forceinline__ double key(const float* v, int a) { return ((double)v[a] + (double)v[3 + a] + (double)v[6 + a]) * (1.0 / 3.0); }
    static __device__ __forceinline__ void put(const Layout& y, int64_t s, int64_t id, const float* v) {
        y.ids[s] = (int)id;
#pragma unroll
        for (int k = 0; k < 9; ++k) y.stri[s * 9 + k] = v[k];
    }
    static __device__ __forceinline__ void grow(const Layout& y, int64_t s, float* lo, float* hi) {     // the box around sorted s too
#pragma unroll
        for (int k = 0; k < 9; ++k) { const float f = y.stri[s * 9 + k]; lo[k % 3] = fminf(lo[k % 3], f); hi[k % 3] = fmaxf(hi[k % 3], f); }
    }
};
struct PointPrim {                               // a point
    static constexpr int kFloats = 3;
    using Layout = GwCloudLayout;
    static Layout carve(const void* index, int64_t n) { return gw_carve_cloud(index, n); }
    static __device__ __forceinline__ double key(const float* v, int a) { return (double)v[a]; }
    static __device__ __forceinline__ void put(const Layout& y, int64_t s, int64_t, const float* v) { y.rows[s] = make_float4(v[0], v[1], v[2], 0.f); }
    static __device__ __forceinline__ void grow(const Layout& y, int64_t s, float* lo, float* hi) {
        const float4 q = y.rows[s];
        lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
        hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
    }
};

// header words 0..2 = min, 3..5 = max of the n points of a flat float3 array (encoded; a soup is its 3 T vertices), 6 = flags
__global__ __launch_bounds__(256) void bvh_bounds_kernel(const float* __restrict__ pos, int64_t n, unsigned* __restrict__ hdr) {
    __shared__ float smin[3][256], smax[3][256];
    __shared__ unsigned sflag;
    if (threadIdx.x == 0) sflag = 0;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool bad = false;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2]};
        bad |= !finite3(v[0], v[1], v[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], v[k]); hi[k] = fmaxf(hi[k], v[k]); }
    }
    __syncthreads();
    if (bad) atomicOr(&sflag, kBvhFlagNonFinite);
#pragma unroll
    for (int a = 0; a < 3; ++a) { smin[a][threadIdx.x] = lo[a]; smax[a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                smin[a][threadIdx.x] = fminf(smin[a][threadIdx.x], smin[a][threadIdx.x + s]);
                smax[a][threadIdx.x] = fmaxf(smax[a][threadIdx.x], smax[a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        atomicMin(&hdr[threadIdx.x], float_code(smin[threadIdx.x][0]));
        atomicMax(&hdr[3 + threadIdx.x], float_code(smax[threadIdx.x][0]));
    }
    if (threadIdx.x == 0 && sflag) atomicOr(&hdr[kBvhHdrFlags], sflag);
}

__device__ __forceinline__ unsigned long long spread21(unsigned long long x) {         // bit i -> bit 3 i
    x &= 0x1fffffull;
    x = (x | (x << 32)) & 0x1f00000000ffffull;
    x = (x | (x << 16)) & 0x1f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

template <class P>
__global__ __launch_bounds__(256) void bvh_codes_kernel(const float* __restrict__ prim, int64_t n, const unsigned* __restrict__ hdr,
                                                        int64_t* __restrict__ codes) {
    double lo[3], ext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = code_float(hdr[a]); ext[a] = (double)code_float(hdr[3 + a]) - lo[a]; }
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const float* v = prim + t * P::kFloats;
        unsigned long long code = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double c = P::key(v, a);
            double q = ext[a] > 0.0 ? (c - lo[a]) / ext[a] * 2097152.0 : 0.0;
            if (!(q >= 0.0)) q = 0.0;                                 // also NaN (the build is refused anyway: header flag)
            if (q > 2097151.0) q = 2097151.0;
            code |= spread21((unsigned long long)q) << (2 - a);       // x in the most significant position
        }
        codes[t] = (int64_t)code;
    }
}

template <class P>
__global__ __launch_bounds__(256) void bvh_gather_kernel(const float* __restrict__ prim, int64_t n, const int64_t* __restrict__ order,
                                                         typename P::Layout y) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        int64_t id = order[s];
        if (id < 0 || id >= n) { atomicOr(&y.hdr[kBvhHdrFlags], kBvhFlagBadOrder); id = 0; }      // not dereferenced; the build is refused
        P::put(y, s, id, prim + id * P::kFloats);
    }
}

// leaf slot j -> node L - 1 + j: the box of sorted primitives [8 j, 8 j + 8), empty past the last primitive
template <class P>
__global__ __launch_bounds__(256) void bvh_leaves_kernel(typename P::Layout y, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < y.L; j += (int64_t)gridDim.x * blockDim.x) {
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        for (int64_t s = j * kBvhLeaf; s < n && s < (j + 1) * kBvhLeaf; ++s) P::grow(y, s, lo, hi);
        store_box(y.nodes, (int64_t)y.L - 1 + j, lo, hi);
    }
}

// nodes [first, first + count) of one level from their children on the level below
__global__ __launch_bounds__(256) void bvh_level_kernel(float4* __restrict__ nodes, int first, int count) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const int64_t n = (int64_t)first + i;
        const float4 a0 = nodes[2 * (2 * n + 1)], a1 = nodes[2 * (2 * n + 1) + 1], b0 = nodes[2 * (2 * n + 2)], b1 = nodes[2 * (2 * n + 2) + 1];
        const float lo[3] = {fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z)};
        const float hi[3] = {fmaxf(a0.w, b0.w), fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y)};
        store_box(nodes, n, lo, hi);
    }
}

template <class P>
size_t bvh_index_bytes(int64_t n) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
    return P::carve(nullptr, n).total;
}

// what both entry points of a build check, in this order; `other` = the codes to write or the order to read
template <class P>
int check_build(const float* prim, int64_t n, const void* other, const void* index, size_t index_bytes) {
    if (n <= 0 || !prim || !other) return DUDF_E_BADCFG;
    if (n >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    return dudf_check_buffer(index, index_bytes, P::carve(nullptr, n).total);
}

// header: bounds of all coordinates and the non-finite flag; clears the other flags
template <class P>
int launch_bounds(const float* prim, int64_t n, unsigned* hdr, hipStream_t st) {
    DUDF_TRY(hipMemsetAsync(hdr, 0, kBvhHdrBytes, st));                       // max words 0 (below every encoded float), flags 0
    DUDF_TRY(hipMemsetAsync(hdr, 0xff, 3 * sizeof(unsigned), st));            // min words above every encoded float
    const int64_t points = n * (P::kFloats / 3);
    return dudf_launch(bvh_bounds_kernel, dim3(dudf_grid_for(points, 256, 256)), dim3(256), st, prim, points, hdr);
}

template <class P>
int bvh_morton_codes(const float* prim, int64_t n, void* index, size_t index_bytes, int64_t* codes, void* stream) {
    if (int rc = check_build<P>(prim, n, codes, index, index_bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    unsigned* hdr = P::carve(index, n).hdr;
    DUDF_TRY(launch_bounds<P>(prim, n, hdr, st));
    return dudf_launch(bvh_codes_kernel<P>, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), st, prim, n, hdr, codes);
}

template <class P>
int bvh_index_build(const float* prim, int64_t n, const int64_t* order, void* index, size_t index_bytes, void* stream) {
    if (int rc = check_build<P>(prim, n, order, index, index_bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const typename P::Layout y = P::carve(index, n);
    DUDF_TRY(launch_bounds<P>(prim, n, y.hdr, st));                           // the build stands alone: any permutation is a valid order
    DUDF_TRY(dudf_launch(bvh_gather_kernel<P>, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), st, prim, n, order, y));
    DUDF_TRY(dudf_launch(bvh_leaves_kernel<P>, dim3(dudf_grid_for(y.L, 256, kGridCap)), dim3(256), st, y, n));
    for (int count = y.L / 2; count >= 1; count /= 2)                         // level of `count` nodes starts at node count - 1
        DUDF_TRY(dudf_launch(bvh_level_kernel, dim3(dudf_grid_for(count, 256, kGridCap)), dim3(256), st, y.nodes, count - 1, count));
    return 0;
}

}  // namespace

extern "C" {

size_t dudf_mesh_index_bytes(int64_t n_tri) { return bvh_index_bytes<TriPrim>(n_tri); }
int dudf_mesh_morton_codes(const float* tri, int64_t n_tri, void* index, size_t index_bytes, int64_t* codes, void* stream) {
    return bvh_morton_codes<TriPrim>(tri, n_tri, index, index_bytes, codes, stream);
}
int dudf_mesh_index_build(const float* tri, int64_t n_tri, const int64_t* order, void* index, size_t index_bytes, void* stream) {
    return bvh_index_build<TriPrim>(tri, n_tri, order, index, index_bytes, stream);
}

size_t dudf_cloud_index_bytes(int64_t n_pc) { return bvh_index_bytes<PointPrim>(n_pc); }
int dudf_cloud_morton_codes(const float* pc_pos, int64_t n_pc, void* index, size_t index_bytes, int64_t* codes, void* stream) {
    return bvh_morton_codes<PointPrim>(pc_pos, n_pc, index, index_bytes, codes, stream);
}
int dudf_cloud_index_build(const float* pc_pos, int64_t n_pc, const int64_t* order, void* index, size_t index_bytes, void* stream) {
    return bvh_index_build<PointPrim>(pc_pos, n_pc, order, index, index_bytes, stream);
}

}  // extern "C"
