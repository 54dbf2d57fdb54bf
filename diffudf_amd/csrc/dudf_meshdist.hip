// Exact unsigned distance from points to a triangle mesh, sub-linear in the number of triangles — what open3d's
// `RaycastingScene.add_triangles / compute_distance` does for reference generate_df.py:108-110 (ground truth of the field slice) —,
// occupancy by ray parity and the sphere-tracing march against the mesh.
// Kernels and their C entry points (include/dudf_hip.h).
//
// The index — a bounding-volume hierarchy without pointers, leaves of 8 sorted triangles — is dudf_bvh.h's; dudf_bvh.hip builds it.
//
// Query: one lane per point, depth-first with a per-lane stack in LDS ([entry][lane]: conflict-free), nearer child first.
//   A subtree is skipped only on the safe-side test of dudf_bvh.h (box_lb > bound_of), so a skipped box holds no triangle at or
//   below the best exact value so far — equal distances are still evaluated and the smallest original index wins.
//   Every triangle evaluation is the fp64 Voronoi-region arithmetic of dudf_tridist.h, called through ONE non-inlined function by
//   the indexed and the brute-force kernel alike: the same machine code, hence the same bits.  The answer is the minimum of those
//   values over a set that contains every minimiser, so the index changes what is skipped, never what is returned.
//
// On the same index: the march of the reference's ground-truth renderer (src/render_st.py:255-268) as one kernel — a ray keeps
// its position in registers and runs the walk above once per iteration (walk_nearest, shared with mesh_distance_kernel) — and
// inside / outside by the parity of the triangles a +x ray crosses (`compute_occupancy`, behind `compute_signed_distance`): a
// walk that visits the boxes the ray meets and one non-inlined crossing test whose edge functions are antisymmetric by
// construction (eval_cross, edge_fn).
#include "dudf_bvh.h"
#include "dudf_tridist.h"

namespace {

constexpr int kBlock = 256;                      // threads per workgroup of the query kernels

// The one copy of the exact evaluation every distance kernel calls (see the head of the file).
__device__ __noinline__ double eval_tri(double px, double py, double pz, const float* t) { return tri_dist2(px, py, pz, t); }

struct MeshView {                     // the soup and, when there is an index, its sections
    const float* tri;                 // the caller's soup (brute force, closest point)
    const int* ids; const float* stri; const float4* nodes;
    int64_t T; int L, depth;
};

struct QueryArgs {
    MeshView m;
    const float* pts; int64_t Q;
    float* dist; int64_t* idx; float* closest; unsigned long long* stats;
};

#define DUDF_TAKE(d2, id) if ((d2) < best || ((d2) == best && (id) < best_id)) { best = (d2); best_id = (id); }

// Nearest triangle of one finite point by a scan of the whole soup: best = the minimum of eval_tri, best_id the smallest index that
// attains it.
__device__ __forceinline__ void scan_nearest(const MeshView& m, float fx, float fy, float fz, double& best, int& best_id) {
    const double px = fx, py = fy, pz = fz;
    for (int64_t t = 0; t < m.T; ++t) {
        const double d2 = eval_tri(px, py, pz, m.tri + t * 9);
        DUDF_TAKE(d2, (int)t)
    }
}

// The same through the index: the depth-first walk of the head of the file.  snode / slb: this lane's column of the [entry][lane]
// stacks (entry e at [e * kBlock]).  evals += exact evaluations.
__device__ __forceinline__ void walk_nearest(const MeshView& m, int* snode, float* slb, float fx, float fy, float fz, double& best,
                                             int& best_id, unsigned long long& evals) {
    const double px = fx, py = fy, pz = fz;
    float bestf = __builtin_inff();
    const int first_leaf = m.L - 1;
    int node = 0, sp = 0;
    for (;;) {                                    // every node is entered at most once: the walk ends whatever the numbers are
        bool pop = true;
        if (node >= first_leaf) {
            const int64_t s0 = (int64_t)(node - first_leaf) * kBvhLeaf;
            const int64_t s1 = (m.T - s0 < kBvhLeaf) ? m.T : s0 + kBvhLeaf;
            for (int64_t s = s0; s < s1; ++s) {
                const double d2 = eval_tri(px, py, pz, m.stri + s * 9);
                const int id = m.ids[s];
                DUDF_TAKE(d2, id)
                ++evals;
            }
            bestf = bound_of(best);
        } else {
            const float4* c = m.nodes + 2 * (2 * (int64_t)node + 1);
            const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
            float ln = box_lb(l0, l1, fx, fy, fz), lf = box_lb(r0, r1, fx, fy, fz);
            int nn = 2 * node + 1, nf = nn + 1;
            if (lf < ln) { const float t = ln; ln = lf; lf = t; nn = nf; nf = nn - 1; }
            if (!(ln > bestf)) {                  // the nearer child may hold the answer; the farther one waits on the stack
                if (!(lf > bestf)) { snode[sp * kBlock] = nf; slb[sp * kBlock] = lf; ++sp; }
                node = nn; pop = false;
            }
        }
        if (pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                if (!(slb[sp * kBlock] > bestf)) { node = snode[sp * kBlock]; found = true; break; }
            }
            if (!found) break;
        }
    }
}

#undef DUDF_TAKE

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
            const float* t = a.m.tri + (int64_t)best_id * 9;
            double cx, cy, cz;
            tri_closest(px, py, pz, t, cx, cy, cz);
            c[0] = (float)(t[0] + cx); c[1] = (float)(t[1] + cy); c[2] = (float)(t[2] + cz);
        }
        a.closest[q * 3] = c[0]; a.closest[q * 3 + 1] = c[1]; a.closest[q * 3 + 2] = c[2];
    }
}

__global__ __launch_bounds__(kBlock) void mesh_distance_brute_kernel(QueryArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = q < a.Q;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (live) { fx = a.pts[q * 3]; fy = a.pts[q * 3 + 1]; fz = a.pts[q * 3 + 2]; }
    const bool nan = fx != fx || fy != fy || fz != fz;
    double best = __builtin_inf(); int best_id = -1;
    unsigned long long evals = 0;
    if (live && !nan) {
        scan_nearest(a.m, fx, fy, fz, best, best_id);
        evals = (unsigned long long)a.m.T;
    }
    finish(a, q, live, nan, fx, fy, fz, best, best_id, evals);
}

__global__ __launch_bounds__(kBlock) void mesh_distance_kernel(QueryArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* snode = reinterpret_cast<int*>(smem) + threadIdx.x;                                      // [depth][kBlock]
    float* slb = reinterpret_cast<float*>(smem) + (size_t)a.m.depth * kBlock + threadIdx.x;       // [depth][kBlock]
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = q < a.Q;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (live) { fx = a.pts[q * 3]; fy = a.pts[q * 3 + 1]; fz = a.pts[q * 3 + 2]; }
    const bool nan = fx != fx || fy != fy || fz != fz;
    double best = __builtin_inf(); int best_id = -1;
    unsigned long long evals = 0;
    if (live && !nan) walk_nearest(a.m, snode, slb, fx, fy, fz, best, best_id, evals);
    finish(a, q, live, nan, fx, fy, fz, best, best_id, evals);
}

// ---- the march of reference src/render_st.py:255-268 against the mesh, one lane per ray -------------------------------------------
// Per iteration of a live ray, in the reference's order: d = the fp32 distance of float32(t0) (what dudf_mesh_distance writes for
// that point: the same walk or scan, the same eval_tri, the same rounding of sqrt); t0 += ray * (double)d, product and sum rounded
// separately; hit when d < float32(surface_eps) — numpy compares the float32 distances with the Python float in float32 —; a ray
// that did not hit dies once a coordinate is outside (-bound, bound).  A NaN position gives d = NaN: no hit, and the ray dies on
// the bound test.  Rays do not depend on each other, so the loop is inside the kernel; a lane leaves it when its ray is done and
// a wave ends when all its lanes have.  No barrier anywhere: lanes past N return at once.
template <bool kIndexed>
__global__ __launch_bounds__(kBlock) void mesh_trace_kernel(MeshView m, const double* __restrict__ rays, double* __restrict__ t0,
                                                            unsigned char* __restrict__ mask, unsigned char* __restrict__ hits,
                                                            int64_t N, float eps, int max_iterations, double bound) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* snode = reinterpret_cast<int*>(smem) + threadIdx.x;
    float* slb = reinterpret_cast<float*>(smem) + (size_t)m.depth * kBlock + threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= N) return;
    const double rx = rays[r * 3], ry = rays[r * 3 + 1], rz = rays[r * 3 + 2];
    double x = t0[r * 3], y = t0[r * 3 + 1], z = t0[r * 3 + 2];
    bool live = mask[r] != 0, hit = false;
    for (int it = 0; it < max_iterations && live; ++it) {
        const float fx = (float)x, fy = (float)y, fz = (float)z;
        float d = __builtin_nanf("");
        if (!(fx != fx || fy != fy || fz != fz)) {
            double best = __builtin_inf(); int best_id = -1;
            if (kIndexed) { unsigned long long evals = 0; walk_nearest(m, snode, slb, fx, fy, fz, best, best_id, evals); }
            else scan_nearest(m, fx, fy, fz, best, best_id);
            d = (float)sqrt(best);
        }
        const double step = (double)d;
        x = x + rx * step; y = y + ry * step; z = z + rz * step;
        if (d < eps) { hit = true; live = false; }
        else if (!(x > -bound && x < bound && y > -bound && y < bound && z > -bound && z < bound)) live = false;
    }
    t0[r * 3] = x; t0[r * 3 + 1] = y; t0[r * 3 + 2] = z;
    mask[r] = live ? 1 : 0;
    hits[r] = hit ? 1 : 0;
}

// ---- occupancy by ray parity: how many triangles the ray from p along +x crosses ----------------------------------------------------
// The ray is axis-aligned, so a crossing is a 2-D point-in-triangle test of (p.y, p.z) in the triangle's projection, on the fp32
// inputs themselves, and then one comparison of the crossing's x with p.x.
//
// Order of two vertices: lexicographic on (y, z, x) as floats — the order of their bits with -0 folded into +0.
__device__ __forceinline__ bool vert_before(const float* a, const float* b) {
    if (a[1] != b[1]) return a[1] < b[1];
    if (a[2] != b[2]) return a[2] < b[2];
    return a[0] <= b[0];
}

// Edge function of (py, pz) for the directed edge a -> b of a triangle: > 0 on the left of it in the (y, z) plane.  It is ALWAYS
// evaluated from the edge's lower vertex to its higher one (one sequence of fp64 roundings, contraction off) and negated when the
// triangle runs the other way, so the two triangles on a shared edge get exactly opposite values whatever was rounded.
// left: the side the point is counted on.  THE TIE RULE: a zero lies on the LEFT of the edge taken from its lower to its higher
// vertex — hence on the right for the triangle that runs it the other way.  With exact values that is the side of the point
// (py - e^2, pz + e), e -> 0+: a footprint is open at its low-y and high-z borders and closed at its high-y and low-z ones.
__device__ __forceinline__ double edge_fn(const float* a, const float* b, double py, double pz, bool& left) {
#pragma clang fp contract(off)
    const bool fwd = vert_before(a, b);
    const float* lo = fwd ? a : b;
    const float* hi = fwd ? b : a;
    const double ly = lo[1], lz = lo[2];
    const double e = ((double)hi[1] - ly) * (pz - lz) - ((double)hi[2] - lz) * (py - ly);
    left = fwd ? (e >= 0.0) : !(e >= 0.0);
    return fwd ? e : -e;
}

// 1 when the ray from p along +x crosses triangle t, else 0 — the one copy the indexed and the brute-force kernel call.
// First the triangle's own box, by the compares the walk applies to a node's box (a node's box contains its triangles' boxes, so
// the walk skips nothing this test would count).  Then: zero projected area counts 0; the three sides must agree; the crossing's x,
// interpolated in fp64 with the edge functions as weights, must be > p.x.
__device__ __noinline__ int eval_cross(float px, float py, float pz, const float* t) {
#pragma clang fp contract(off)
    const float ylo = fminf(fminf(t[1], t[4]), t[7]), yhi = fmaxf(fmaxf(t[1], t[4]), t[7]);
    const float zlo = fminf(fminf(t[2], t[5]), t[8]), zhi = fmaxf(fmaxf(t[2], t[5]), t[8]);
    const float xhi = fmaxf(fmaxf(t[0], t[3]), t[6]);
    if (!(py >= ylo && py <= yhi && pz >= zlo && pz <= zhi && xhi >= px)) return 0;
    const double y = py, z = pz;
    const double y0 = t[1], z0 = t[2];
    const double area2 = ((double)t[4] - y0) * ((double)t[8] - z0) - ((double)t[5] - z0) * ((double)t[7] - y0);
    if (area2 == 0.0) return 0;
    bool s0, s1, s2;
    const double e0 = edge_fn(t, t + 3, y, z, s0);               // weight of vertex 2
    const double e1 = edge_fn(t + 3, t + 6, y, z, s1);           // weight of vertex 0
    const double e2 = edge_fn(t + 6, t, y, z, s2);               // weight of vertex 1
    if (s0 != s1 || s1 != s2) return 0;
    const double sum = (e0 + e1) + e2;
    if (sum == 0.0) return 0;
    const double x = ((e1 * (double)t[0] + e2 * (double)t[3]) + e0 * (double)t[6]) / sum;
    return x > (double)px ? 1 : 0;
}

struct OccArgs {
    MeshView m;
    const float* pts; int64_t Q;
    int* count; unsigned char* inside;
};

__device__ __forceinline__ void finish_occ(const OccArgs& a, int64_t q, bool nan, int count) {
    if (a.count) a.count[q] = nan ? -1 : count;
    if (a.inside) a.inside[q] = nan ? 0 : (unsigned char)(count & 1);
}

__global__ __launch_bounds__(kBlock) void mesh_occupancy_brute_kernel(OccArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.Q) return;
    const float fx = a.pts[q * 3], fy = a.pts[q * 3 + 1], fz = a.pts[q * 3 + 2];
    const bool nan = fx != fx || fy != fy || fz != fz;
    int count = 0;
    if (!nan)
        for (int64_t t = 0; t < a.m.T; ++t) count += eval_cross(fx, fy, fz, a.m.tri + t * 9);
    finish_occ(a, q, nan, count);
}

// a box is visited iff (p.y, p.z) lies in its closed (y, z) extent and its hi.x >= p.x: compares on stored floats, no tolerance
__device__ __forceinline__ bool box_on_ray(const float4& b0, const float4& b1, float px, float py, float pz) {
    return py >= b0.y && py <= b1.x && pz >= b0.z && pz <= b1.y && b0.w >= px;
}

// One lane per point, depth-first; a lane pushes at most one node per level, so the [entry][lane] stack of mesh_distance_kernel
// (its node half) is deep enough.  The count is a sum over the visited leaves: the order of visits does not matter.
__global__ __launch_bounds__(kBlock) void mesh_occupancy_kernel(OccArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* snode = reinterpret_cast<int*>(smem) + threadIdx.x;                                      // [depth][kBlock]
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.Q) return;                                         // no barrier in this kernel
    const float fx = a.pts[q * 3], fy = a.pts[q * 3 + 1], fz = a.pts[q * 3 + 2];
    const bool nan = fx != fx || fy != fy || fz != fz;
    int count = 0;
    if (!nan) {
        const int first_leaf = a.m.L - 1;
        int node = 0, sp = 0;
        bool go = true;
        if (first_leaf > 0) {                                     // the root's own box is stored too: test it like any other
            const float4* c = a.m.nodes;
            go = box_on_ray(c[0], c[1], fx, fy, fz);
        }
        while (go) {                                              // every node is entered at most once
            bool pop = true;
            if (node >= first_leaf) {
                const int64_t s0 = (int64_t)(node - first_leaf) * kBvhLeaf;
                const int64_t s1 = (a.m.T - s0 < kBvhLeaf) ? a.m.T : s0 + kBvhLeaf;
                for (int64_t s = s0; s < s1; ++s) count += eval_cross(fx, fy, fz, a.m.stri + s * 9);
            } else {
                const float4* c = a.m.nodes + 2 * (2 * (int64_t)node + 1);
                const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
                const bool hl = box_on_ray(l0, l1, fx, fy, fz), hr = box_on_ray(r0, r1, fx, fy, fz);
                if (hl || hr) {
                    if (hl && hr) { snode[sp * kBlock] = 2 * node + 2; ++sp; }
                    node = hl ? 2 * node + 1 : 2 * node + 2; pop = false;
                }
            }
            if (pop) {
                if (sp == 0) break;
                --sp; node = snode[sp * kBlock];
            }
        }
    }
    finish_occ(a, q, nan, count);
}

}  // namespace

extern "C" {

// a query accepts any buffer that holds the index: there, aligned, at least the published size
static int check_index(const void* index, size_t index_bytes, int64_t T) { return dudf_check_buffer(index, index_bytes, gw_carve_mesh(nullptr, T).total); }

// the soup alone (index == NULL: the kernels scan it) or with the sections of its index
static MeshView view_of(const float* tri, int64_t n_tri, const void* index) {
    MeshView m;
    m.tri = tri; m.T = n_tri; m.ids = nullptr; m.stri = nullptr; m.nodes = nullptr; m.L = 0; m.depth = 0;
    if (index) {
        const GwMeshLayout y = gw_carve_mesh(index, n_tri);
        m.ids = y.ids; m.stri = y.stri; m.nodes = y.nodes; m.L = y.L; m.depth = y.depth;
    }
    return m;
}

// what every query checks, in this order; n = points or rays.  > 0: nothing to do (n == 0)
static int check_query(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const void* in, int64_t n) {
    if (n < 0) return DUDF_E_BADCFG;
    if (n == 0) return 1;
    if (n_tri <= 0 || !tri || !in) return DUDF_E_BADCFG;
    if (n_tri >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (index && check_index(index, index_bytes, n_tri)) return DUDF_E_WORKSPACE;
    if ((n + kBlock - 1) / kBlock >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    return 0;
}

int dudf_mesh_distance(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const float* pts, int64_t n_pts,
                       float* out_dist, int64_t* out_tri, float* out_closest, int64_t* out_stats, void* stream) {
    if (int rc = check_query(tri, n_tri, index, index_bytes, pts, n_pts)) return rc > 0 ? 0 : rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    QueryArgs a;
    a.m = view_of(tri, n_tri, index); a.pts = pts; a.Q = n_pts;
    a.dist = out_dist; a.idx = out_tri; a.closest = out_closest; a.stats = reinterpret_cast<unsigned long long*>(out_stats);
    const dim3 grid((unsigned)((n_pts + kBlock - 1) / kBlock));
    if (!index) return dudf_launch(mesh_distance_brute_kernel, grid, dim3(kBlock), st, a);
    const size_t lds = (size_t)a.m.depth * kBlock * (sizeof(int) + sizeof(float));      // <= 29 * 2 KiB
    return dudf_launch_lds(mesh_distance_kernel, grid, dim3(kBlock), lds, st, a);
}

int dudf_mesh_occupancy(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const float* pts, int64_t n_pts,
                        int32_t* out_count, unsigned char* out_inside, void* stream) {
    if (int rc = check_query(tri, n_tri, index, index_bytes, pts, n_pts)) return rc > 0 ? 0 : rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    OccArgs a;
    a.m = view_of(tri, n_tri, index); a.pts = pts; a.Q = n_pts; a.count = out_count; a.inside = out_inside;
    const dim3 grid((unsigned)((n_pts + kBlock - 1) / kBlock));
    if (!index) return dudf_launch(mesh_occupancy_brute_kernel, grid, dim3(kBlock), st, a);
    const size_t lds = (size_t)a.m.depth * kBlock * sizeof(int);
    return dudf_launch_lds(mesh_occupancy_kernel, grid, dim3(kBlock), lds, st, a);
}

int dudf_mesh_trace_rays(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const double* rays, double* t0,
                         unsigned char* mask, unsigned char* hits, int64_t n_rays, double surface_eps, int max_iterations,
                         double bound, void* stream) {
    if (int rc = check_query(tri, n_tri, index, index_bytes, rays, n_rays)) return rc > 0 ? 0 : rc;
    if (!t0 || !mask || !hits || max_iterations < 0) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const MeshView m = view_of(tri, n_tri, index);
    const dim3 grid((unsigned)((n_rays + kBlock - 1) / kBlock));
    if (!index)
        return dudf_launch(mesh_trace_kernel<false>, grid, dim3(kBlock), st, m, rays, t0, mask, hits, n_rays, (float)surface_eps,
                           max_iterations, bound);
    const size_t lds = (size_t)m.depth * kBlock * (sizeof(int) + sizeof(float));
    return dudf_launch_lds(mesh_trace_kernel<true>, grid, dim3(kBlock), lds, st, m, rays, t0, mask, hits, n_rays, (float)surface_eps,
                           max_iterations, bound);
}

}  // extern "C"
