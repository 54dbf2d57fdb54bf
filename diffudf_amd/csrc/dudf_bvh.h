// The index of the mesh-distance queries (dudf_meshdist.hip) and of the indexed batch sampler (dudf_sample_indexed.hip): its format
// and the pruning arithmetic of every walk, stated once.  dudf_bvh.hip builds it.  Host layouts and device code; internal.
//
// A bounding-volume hierarchy without pointers, over triangles (the mesh index) or points (the cloud index):
//   - Morton code (3 x 21 bits) of every primitive — a triangle's centroid, a point — inside the bounding box of all of them; the
//     caller sorts the codes (stable) and hands the order back;
//   - the sorted primitives are copied once: triangles as 9 floats next to their original indices (a leaf's triangles are then 288
//     contiguous bytes), points as 16-byte rows (x, y, z, 0);
//   - leaf j holds sorted primitives [8 j, 8 j + 8); the leaves are the last level of a complete binary tree in heap order
//     (node i has children 2 i + 1 and 2 i + 2) over L = the next power of two of the leaf count; slots past the last leaf
//     carry an empty box (lo = +inf, hi = -inf) that no query ever finds near;
//   - a node is its fp32 AABB, two float4 (lo.xyz hi.x | hi.yz 0 0): min / max of fp32 coordinates, exact.  One kernel per level.
// Everything is a function of (primitives, order): two builds give the same bytes (tests/test_index_bytes_gpu.py pins them).
//
// A walk skips a subtree only when  lb * 0.99999 > best * 1.00001 + tiny  in fp32, lb the squared distance to its box: the fp32 box
// distance is within a few 2^-24 of the true one and the factors cover that many times over, so a skipped box holds no primitive
// at or below the best exact value so far.  box_lb / bound_of below are that test's two sides, for the one-lane walk of
// dudf_meshdist.hip and the grouped walk of dudf_groupwalk.h alike: "index == brute force, bit for bit" rests on them.
#ifndef DUDF_BVH_H
#define DUDF_BVH_H
#include "dudf_context.h"
#include "dudf_pairdist.h"         // float_code / code_float of the header's bounds, finite3

constexpr int kBvhLeaf = 8;                           // primitives per leaf
constexpr int kBvhHdrBytes = 256;                     // header: words 0..2 = min, 3..5 = max of all coordinates (float_code), 6 = flags
constexpr int kBvhHdrFlags = 6;                       // (byte DUDF_MESH_INDEX_FLAGS_OFFSET)
constexpr unsigned kBvhFlagNonFinite = DUDF_MESH_FLAG_NONFINITE, kBvhFlagBadOrder = DUDF_MESH_FLAG_BAD_ORDER;
static_assert(kBvhHdrFlags * sizeof(unsigned) == DUDF_MESH_INDEX_FLAGS_OFFSET, "the published place of the flag word");

// L leaf slots (a power of two) and the stack entries a walk can need for n primitives
inline void gw_shape(int64_t n, int& L, int& depth) {
    const int64_t leaves = (n + kBvhLeaf - 1) / kBvhLeaf;
    int lg = 0;
    while (((int64_t)1 << lg) < leaves) ++lg;
    L = 1 << lg; depth = lg + 1;
}

// the published layout of the mesh index: header, ids [T], sorted triangles [T][9], nodes [2L - 1][2], each on a 256-byte granule
// (sections null for a null index, `total` its size)
struct GwMeshLayout { unsigned* hdr; int* ids; float* stri; float4* nodes; int L, depth; size_t total; };
inline GwMeshLayout gw_carve_mesh(const void* index, int64_t T) {
    GwMeshLayout y;
    gw_shape(T, y.L, y.depth);
    DudfByteCarver cv = dudf_carve(index);
    y.hdr = cv.take<unsigned>(kBvhHdrBytes / sizeof(unsigned));
    y.ids = cv.take<int>(T); y.stri = cv.take<float>(T * 9); y.nodes = cv.take<float4>((2 * (int64_t)y.L - 1) * 2);
    y.total = cv.o;
    return y;
}
// ... and of the cloud index: header, sorted points [n] as (x, y, z, 0), nodes [2L - 1][2]
struct GwCloudLayout { unsigned* hdr; float4* rows; float4* nodes; int L, depth; size_t total; };
inline GwCloudLayout gw_carve_cloud(const void* index, int64_t n) {
    GwCloudLayout y;
    gw_shape(n, y.L, y.depth);
    DudfByteCarver cv = dudf_carve(index);
    y.hdr = cv.take<unsigned>(kBvhHdrBytes / sizeof(unsigned));
    y.rows = cv.take<float4>(n); y.nodes = cv.take<float4>((2 * (int64_t)y.L - 1) * 2);
    y.total = cv.o;
    return y;
}

__device__ __forceinline__ void store_box(float4* __restrict__ nodes, int64_t node, const float* lo, const float* hi) {
    nodes[2 * node] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    nodes[2 * node + 1] = make_float4(hi[1], hi[2], 0.f, 0.f);
}

// safe-side fp32 lower bound of the squared distance from p to a box (0 inside; +inf for an empty box)
__device__ __forceinline__ float box_lb(const float4& b0, const float4& b1, float px, float py, float pz) {
    const float dx = fmaxf(fmaxf(b0.x - px, px - b0.w), 0.f);
    const float dy = fmaxf(fmaxf(b0.y - py, py - b1.x), 0.f);
    const float dz = fmaxf(fmaxf(b0.z - pz, pz - b1.y), 0.f);
    return (dx * dx + dy * dy + dz * dz) * 0.99999f;
}
// fp32 upper bound of the best exact squared distance
__device__ __forceinline__ float bound_of(double best) { return (float)best * 1.00001f + 1e-37f; }

#endif  // DUDF_BVH_H
