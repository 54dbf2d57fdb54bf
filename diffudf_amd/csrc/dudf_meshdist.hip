// Exact unsigned distance from points to a triangle mesh, sub-linear in the number of triangles — what open3d's
// `RaycastingScene.add_triangles / compute_distance` does for reference generate_df.py:108-110 (ground truth of the field slice).
// Kernels and their C entry points (include/dudf_hip.h).
//
// Index: a bounding-volume hierarchy without pointers.
//   - Morton code (3 x 21 bits) of every triangle's centroid inside the mesh's bounding box; the caller sorts the codes (stable)
//     and hands the order back;
//   - the sorted triangles are copied once (a leaf's triangles are then 288 contiguous bytes) next to their original indices;
//   - leaf j holds sorted triangles [8 j, 8 j + 8); the leaves are the last level of a complete binary tree in heap order
//     (node i has children 2 i + 1 and 2 i + 2) over L = the next power of two of the leaf count; slots past the last leaf
//     carry an empty box (lo = +inf, hi = -inf) that no query ever finds near;
//   - a node is its fp32 AABB, two float4 (lo.xyz hi.x | hi.yz - -): min / max of fp32 vertices, exact.  One kernel per level.
// Everything is a function of (triangles, order): two builds give the same bytes.
//
// Query: one lane per point, depth-first with a per-lane stack in LDS ([entry][lane]: conflict-free), nearer child first.
//   A subtree is skipped only when  lb * 0.99999 > best * 1.00001 + tiny  in fp32, lb the squared distance to its box: the fp32
//   box distance is within a few 2^-24 of the true one and the factors cover that many times over, so a skipped box holds no
//   triangle at or below the best exact value so far — equal distances are still evaluated and the smallest original index wins.
//   Every triangle evaluation is the fp64 Voronoi-region arithmetic of dudf_tridist.h, called through ONE non-inlined function by
//   the indexed and the brute-force kernel alike: the same machine code, hence the same bits.  The answer is the minimum of those
//   values over a set that contains every minimiser, so the index changes what is skipped, never what is returned.
#include "dudf_context.h"
#include "dudf_tridist.h"

namespace {

constexpr int kLeaf = 8;                         // triangles per leaf
constexpr int kBlock = 256;                      // threads per workgroup of the query kernels
constexpr int kHdrBytes = 256;                   // header: 3 + 3 encoded bounds, flags
constexpr unsigned kFlagNonFinite = 1u, kFlagBadOrder = 2u;

struct Layout {                                  // byte offsets inside the index
    int64_t n_leaves; int L, depth;              // L leaf slots (power of two), depth = stack entries a lane can need
    size_t ids, stri, nodes, total;
};
inline size_t round256(size_t b) { return (b + 255) / 256 * 256; }
inline Layout layout_of(int64_t T) {
    Layout y;
    y.n_leaves = (T + kLeaf - 1) / kLeaf;
    int lg = 0;
    while (((int64_t)1 << lg) < y.n_leaves) ++lg;
    y.L = 1 << lg; y.depth = lg + 1;
    y.ids = kHdrBytes;
    y.stri = y.ids + round256((size_t)T * sizeof(int));
    y.nodes = y.stri + round256((size_t)T * 9 * sizeof(float));
    y.total = y.nodes + round256((size_t)(2 * (int64_t)y.L - 1) * 2 * sizeof(float4));
    return y;
}
inline int grid_for(int64_t n, int block = 256, int cap = 8192) {
    int64_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// fp32 -> uint32 whose unsigned order is the float order (for atomicMin / atomicMax of bounds)
__device__ __forceinline__ unsigned enc(float f) { const unsigned b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// header words 0..2 = min, 3..5 = max of all vertices (encoded), 6 = flags
__global__ __launch_bounds__(256) void mesh_bounds_kernel(const float* __restrict__ tri, int64_t T, unsigned* __restrict__ hdr) {
    __shared__ float smin[3][256], smax[3][256];
    __shared__ unsigned sflag;
    if (threadIdx.x == 0) sflag = 0;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool bad = false;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
        const float* v = tri + t * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float f = v[k];
            bad |= !(fabsf(f) <= 3.402823466e38f);                 // NaN or infinity
            lo[k % 3] = fminf(lo[k % 3], f); hi[k % 3] = fmaxf(hi[k % 3], f);
        }
    }
    __syncthreads();
    if (bad) atomicOr(&sflag, kFlagNonFinite);
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
        atomicMin(&hdr[threadIdx.x], enc(smin[threadIdx.x][0]));
        atomicMax(&hdr[3 + threadIdx.x], enc(smax[threadIdx.x][0]));
    }
    if (threadIdx.x == 0 && sflag) atomicOr(&hdr[6], sflag);
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

__global__ __launch_bounds__(256) void mesh_codes_kernel(const float* __restrict__ tri, int64_t T, const unsigned* __restrict__ hdr,
                                                         int64_t* __restrict__ codes) {
    double lo[3], ext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = dec(hdr[a]); ext[a] = (double)dec(hdr[3 + a]) - lo[a]; }
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
        const float* v = tri + t * 9;
        unsigned long long code = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double c = ((double)v[a] + (double)v[3 + a] + (double)v[6 + a]) * (1.0 / 3.0);
            double q = ext[a] > 0.0 ? (c - lo[a]) / ext[a] * 2097152.0 : 0.0;
            if (!(q >= 0.0)) q = 0.0;                                 // also NaN (the build is refused anyway: header flag)
            if (q > 2097151.0) q = 2097151.0;
            code |= spread21((unsigned long long)q) << (2 - a);       // x in the most significant position
        }
        codes[t] = (int64_t)code;
    }
}

__global__ __launch_bounds__(256) void mesh_gather_kernel(const float* __restrict__ tri, int64_t T, const int64_t* __restrict__ order,
                                                          int* __restrict__ ids, float* __restrict__ stri, unsigned* __restrict__ hdr) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T; s += (int64_t)gridDim.x * blockDim.x) {
        int64_t id = order[s];
        if (id < 0 || id >= T) { atomicOr(&hdr[6], kFlagBadOrder); id = 0; }      // not dereferenced; the build is refused
        ids[s] = (int)id;
#pragma unroll
        for (int k = 0; k < 9; ++k) stri[s * 9 + k] = tri[id * 9 + k];
    }
}

__device__ __forceinline__ void store_box(float4* __restrict__ nodes, int64_t node, const float* lo, const float* hi) {
    nodes[2 * node] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    nodes[2 * node + 1] = make_float4(hi[1], hi[2], 0.f, 0.f);
}

// leaf slot j -> node L - 1 + j: the box of sorted triangles [8 j, 8 j + 8), empty past the last triangle
__global__ __launch_bounds__(256) void mesh_leaves_kernel(const float* __restrict__ stri, int64_t T, int L, float4* __restrict__ nodes) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < L; j += (int64_t)gridDim.x * blockDim.x) {
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        for (int64_t s = j * kLeaf; s < T && s < (j + 1) * kLeaf; ++s)
#pragma unroll
            for (int k = 0; k < 9; ++k) { const float f = stri[s * 9 + k]; lo[k % 3] = fminf(lo[k % 3], f); hi[k % 3] = fmaxf(hi[k % 3], f); }
        store_box(nodes, (int64_t)L - 1 + j, lo, hi);
    }
}

// nodes [first, first + count) of one level from their children on the level below
__global__ __launch_bounds__(256) void mesh_level_kernel(float4* __restrict__ nodes, int first, int count) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const int64_t n = (int64_t)first + i;
        const float4 a0 = nodes[2 * (2 * n + 1)], a1 = nodes[2 * (2 * n + 1) + 1], b0 = nodes[2 * (2 * n + 2)], b1 = nodes[2 * (2 * n + 2) + 1];
        const float lo[3] = {fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z)};
        const float hi[3] = {fmaxf(a0.w, b0.w), fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y)};
        store_box(nodes, n, lo, hi);
    }
}

// ---- queries ---------------------------------------------------------------------------------------------------------------------
// The one copy of the exact evaluation both kernels call (see the head of the file).
__device__ __noinline__ double eval_tri(double px, double py, double pz, const float* t) { return tri_dist2(px, py, pz, t); }

struct QueryArgs {
    const float* tri;                 // the caller's soup (brute force, closest point)
    const int* ids; const float* stri; const float4* nodes;
    int64_t T; int L, depth;
    const float* pts; int64_t Q;
    float* dist; int64_t* idx; float* closest; unsigned long long* stats;
};

// safe-side fp32 lower bound of the squared distance from p to a box (0 inside; +inf for an empty box)
__device__ __forceinline__ float box_lb(const float4& b0, const float4& b1, float px, float py, float pz) {
    const float dx = fmaxf(fmaxf(b0.x - px, px - b0.w), 0.f);
    const float dy = fmaxf(fmaxf(b0.y - py, py - b1.x), 0.f);
    const float dz = fmaxf(fmaxf(b0.z - pz, pz - b1.y), 0.f);
    return (dx * dx + dy * dy + dz * dz) * 0.99999f;
}
// fp32 upper bound of the best exact squared distance
__device__ __forceinline__ float bound_of(double best) { return (float)best * 1.00001f + 1e-37f; }

__device__ __forceinline__ void finish(const QueryArgs& a, int64_t q, bool live, bool nan, double px, double py, double pz, double best,
                                       int best_id, unsigned long long evals) {
    if (a.stats) {                                                    // one atomic per wave; integer: order does not matter
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) evals += __shfl_xor(evals, m);
        if ((threadIdx.x & 63) == 0 && evals) atomicAdd(a.stats, evals);
    }
    if (!live) return;
    if (a.dist) a.dist[q] = nan ? __builtin_nanf("") : (float)sqrt(best);
    if (a.idx) a.idx[q] = best_id;
    if (a.closest) {
        float c[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        if (best_id >= 0) {
            const float* t = a.tri + (int64_t)best_id * 9;
            double cx, cy, cz;
            tri_closest(px, py, pz, t, cx, cy, cz);
            c[0] = (float)(t[0] + cx); c[1] = (float)(t[1] + cy); c[2] = (float)(t[2] + cz);
        }
        a.closest[q * 3] = c[0]; a.closest[q * 3 + 1] = c[1]; a.closest[q * 3 + 2] = c[2];
    }
}

#define DUDF_TAKE(d2, id) if ((d2) < best || ((d2) == best && (id) < best_id)) { best = (d2); best_id = (id); }

__global__ __launch_bounds__(kBlock) void mesh_distance_brute_kernel(QueryArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = q < a.Q;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (live) { fx = a.pts[q * 3]; fy = a.pts[q * 3 + 1]; fz = a.pts[q * 3 + 2]; }
    const bool nan = fx != fx || fy != fy || fz != fz;
    const double px = fx, py = fy, pz = fz;
    double best = __builtin_inf(); int best_id = -1;
    unsigned long long evals = 0;
    if (live && !nan) {
        for (int64_t t = 0; t < a.T; ++t) {
            const double d2 = eval_tri(px, py, pz, a.tri + t * 9);
            DUDF_TAKE(d2, (int)t)
        }
        evals = (unsigned long long)a.T;
    }
    finish(a, q, live, nan, px, py, pz, best, best_id, evals);
}

__global__ __launch_bounds__(kBlock) void mesh_distance_kernel(QueryArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* snode = reinterpret_cast<int*>(smem);                                    // [depth][kBlock]
    float* slb = reinterpret_cast<float*>(smem) + (size_t)a.depth * kBlock;       // [depth][kBlock]
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = q < a.Q;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (live) { fx = a.pts[q * 3]; fy = a.pts[q * 3 + 1]; fz = a.pts[q * 3 + 2]; }
    const bool nan = fx != fx || fy != fy || fz != fz;
    const double px = fx, py = fy, pz = fz;
    double best = __builtin_inf(); int best_id = -1;
    float bestf = __builtin_inff();
    unsigned long long evals = 0;
    if (live && !nan) {
        const int first_leaf = a.L - 1;
        int node = 0, sp = 0;
        for (;;) {                                    // every node is entered at most once: the walk ends whatever the numbers are
            bool pop = true;
            if (node >= first_leaf) {
                const int64_t s0 = (int64_t)(node - first_leaf) * kLeaf;
                const int64_t s1 = (a.T - s0 < kLeaf) ? a.T : s0 + kLeaf;
                for (int64_t s = s0; s < s1; ++s) {
                    const double d2 = eval_tri(px, py, pz, a.stri + s * 9);
                    const int id = a.ids[s];
                    DUDF_TAKE(d2, id)
                    ++evals;
                }
                bestf = bound_of(best);
            } else {
                const float4* c = a.nodes + 2 * (2 * (int64_t)node + 1);
                const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
                float ln = box_lb(l0, l1, fx, fy, fz), lf = box_lb(r0, r1, fx, fy, fz);
                int nn = 2 * node + 1, nf = nn + 1;
                if (lf < ln) { const float t = ln; ln = lf; lf = t; nn = nf; nf = nn - 1; }
                if (!(ln > bestf)) {                  // the nearer child may hold the answer; the farther one waits on the stack
                    if (!(lf > bestf)) { snode[sp * kBlock + threadIdx.x] = nf; slb[sp * kBlock + threadIdx.x] = lf; ++sp; }
                    node = nn; pop = false;
                }
            }
            if (pop) {
                bool found = false;
                while (sp > 0) {
                    --sp;
                    if (!(slb[sp * kBlock + threadIdx.x] > bestf)) { node = snode[sp * kBlock + threadIdx.x]; found = true; break; }
                }
                if (!found) break;
            }
        }
    }
    finish(a, q, live, nan, px, py, pz, best, best_id, evals);
}

#undef DUDF_TAKE

}  // namespace

extern "C" {

size_t dudf_mesh_index_bytes(int64_t n_tri) {
    if (n_tri <= 0 || n_tri >= ((int64_t)1 << 31)) return 0;
    return layout_of(n_tri).total;
}

// header: bounds of all vertices and the non-finite flag; clears the other flags
static hipError_t launch_bounds(const float* tri, int64_t T, unsigned* hdr, hipStream_t st) {
    hipError_t e = hipMemsetAsync(hdr, 0, kHdrBytes, st);                     // max words 0 (below every encoded float), flags 0
    if (e == hipSuccess) e = hipMemsetAsync(hdr, 0xff, 3 * sizeof(unsigned), st);   // min words above every encoded float
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mesh_bounds_kernel, dim3(grid_for(T, 256, 256)), dim3(256), 0, st, tri, T, hdr);
    return hipGetLastError();
}

static int check_index(const void* index, size_t index_bytes, int64_t T) { return dudf_check_buffer(index, index_bytes, layout_of(T).total); }

int dudf_mesh_morton_codes(const float* tri, int64_t n_tri, void* index, size_t index_bytes, int64_t* codes, void* stream) {
    if (n_tri <= 0 || !tri || !codes) return DUDF_E_BADCFG;
    if (n_tri >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (int rc = check_index(index, index_bytes, n_tri)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    unsigned* hdr = reinterpret_cast<unsigned*>(index);
    hipError_t e = launch_bounds(tri, n_tri, hdr, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mesh_codes_kernel, dim3(grid_for(n_tri)), dim3(256), 0, st, tri, n_tri, hdr, codes);
    return (int)hipGetLastError();
}

int dudf_mesh_index_build(const float* tri, int64_t n_tri, const int64_t* order, void* index, size_t index_bytes, void* stream) {
    if (n_tri <= 0 || !tri || !order) return DUDF_E_BADCFG;
    if (n_tri >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (int rc = check_index(index, index_bytes, n_tri)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const Layout y = layout_of(n_tri);
    char* base = reinterpret_cast<char*>(index);
    unsigned* hdr = reinterpret_cast<unsigned*>(base);
    int* ids = reinterpret_cast<int*>(base + y.ids);
    float* stri = reinterpret_cast<float*>(base + y.stri);
    float4* nodes = reinterpret_cast<float4*>(base + y.nodes);
    hipError_t e = launch_bounds(tri, n_tri, hdr, st);                        // the build stands alone: any permutation is a valid order
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mesh_gather_kernel, dim3(grid_for(n_tri)), dim3(256), 0, st, tri, n_tri, order, ids, stri, hdr);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mesh_leaves_kernel, dim3(grid_for(y.L)), dim3(256), 0, st, stri, n_tri, y.L, nodes);
    e = hipGetLastError();
    for (int count = y.L / 2; count >= 1 && e == hipSuccess; count /= 2) {       // level of `count` nodes starts at node count - 1
        hipLaunchKernelGGL(mesh_level_kernel, dim3(grid_for(count)), dim3(256), 0, st, nodes, count - 1, count);
        e = hipGetLastError();
    }
    return (int)e;
}

int dudf_mesh_distance(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const float* pts, int64_t n_pts,
                       float* out_dist, int64_t* out_tri, float* out_closest, int64_t* out_stats, void* stream) {
    if (n_pts < 0) return DUDF_E_BADCFG;
    if (n_pts == 0) return 0;
    if (n_tri <= 0 || !tri || !pts) return DUDF_E_BADCFG;
    if (n_tri >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (index && check_index(index, index_bytes, n_tri)) return DUDF_E_WORKSPACE;
    if ((n_pts + kBlock - 1) / kBlock >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    QueryArgs a;
    a.tri = tri; a.T = n_tri; a.pts = pts; a.Q = n_pts;
    a.dist = out_dist; a.idx = out_tri; a.closest = out_closest; a.stats = reinterpret_cast<unsigned long long*>(out_stats);
    a.ids = nullptr; a.stri = nullptr; a.nodes = nullptr; a.L = 0; a.depth = 0;
    const dim3 grid((unsigned)((n_pts + kBlock - 1) / kBlock));
    if (!index) {
        hipLaunchKernelGGL(mesh_distance_brute_kernel, grid, dim3(kBlock), 0, st, a);
        return (int)hipGetLastError();
    }
    const Layout y = layout_of(n_tri);
    const char* base = reinterpret_cast<const char*>(index);
    a.ids = reinterpret_cast<const int*>(base + y.ids);
    a.stri = reinterpret_cast<const float*>(base + y.stri);
    a.nodes = reinterpret_cast<const float4*>(base + y.nodes);
    a.L = y.L; a.depth = y.depth;
    const size_t lds = (size_t)y.depth * kBlock * (sizeof(int) + sizeof(float));      // <= 29 * 2 KiB
    hipLaunchKernelGGL(mesh_distance_kernel, grid, dim3(kBlock), lds, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
