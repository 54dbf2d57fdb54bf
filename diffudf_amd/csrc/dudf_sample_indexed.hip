// The per-step training batch of dudf_sample.hip with its distances taken through an index instead of a scan of the whole shape —
// for meshes and clouds too large for the scan (its cost per step is linear in the triangles / points; the walk's is logarithmic).
// Kernels and their C entry points (include/dudf_hip.h).
//
//   - mesh input: the off-surface samples walk the mesh index dudf_mesh_index_build wrote (leaves of 8 sorted triangles);
//   - cloud input (n_tri == 0): the far samples walk the CLOUD index built here — the same fixed-shape Morton tree over pc_pos:
//     leaves of 8 points, a sorted copy as 16-byte rows, boxes in heap order, one kernel for the leaves and one per level.
// The walk is dudf_groupwalk.h: 8 lanes per sample, a leaf per step.  Samples are the ones of sample_batch_kernel — the same keys,
// strata, sharding and [on | far | near] layout; its generation code is restated here, not shared, so that kernel stays as it is —
// and every distance is the minimum of the same exact fp64 values, so the batch is bit-identical to dudf_sample_batch's
// (tests/test_sampler_indexed_gpu.py).  The launch makes no allocation, copy or synchronisation: it can be captured in a graph.
#include "dudf_groupwalk.h"

#include <type_traits>

#include "dudf_rng.h"              // dudf_splitmix64, dudf_uniform01

namespace {

constexpr int kGridCap = 8192;                   // workgroups of the build launches; the kernels stride over the rest
constexpr unsigned kFlagNonFinite = 1u, kFlagBadOrder = 2u;

// ---- the cloud index ----------------------------------------------------------------------------------------------------------------
// fp32 -> uint32 whose unsigned order is the float order (for atomicMin / atomicMax of bounds)
__device__ __forceinline__ unsigned enc(float f) { const unsigned b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// header words 0..2 = min, 3..5 = max of all points (encoded), 6 = flags
__global__ __launch_bounds__(256) void cloud_bounds_kernel(const float* __restrict__ pos, int64_t n, unsigned* __restrict__ hdr) {
    __shared__ float smin[3][256], smax[3][256];
    __shared__ unsigned sflag;
    if (threadIdx.x == 0) sflag = 0;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool bad = false;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = pos[p * 3 + k];
            bad |= !(fabsf(f) <= 3.402823466e38f);                     // NaN or infinity
            lo[k] = fminf(lo[k], f); hi[k] = fmaxf(hi[k], f);
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

__global__ __launch_bounds__(256) void cloud_codes_kernel(const float* __restrict__ pos, int64_t n, const unsigned* __restrict__ hdr,
                                                          int64_t* __restrict__ codes) {
    double lo[3], ext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = dec(hdr[a]); ext[a] = (double)dec(hdr[3 + a]) - lo[a]; }
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long code = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double q = ext[a] > 0.0 ? ((double)pos[p * 3 + a] - lo[a]) / ext[a] * 2097152.0 : 0.0;
            if (!(q >= 0.0)) q = 0.0;                                 // also NaN (the build is refused anyway: header flag)
            if (q > 2097151.0) q = 2097151.0;
            code |= spread21((unsigned long long)q) << (2 - a);       // x in the most significant position
        }
        codes[p] = (int64_t)code;
    }
}

__global__ __launch_bounds__(256) void cloud_gather_kernel(const float* __restrict__ pos, int64_t n, const int64_t* __restrict__ order,
                                                           float4* __restrict__ rows, unsigned* __restrict__ hdr) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        int64_t id = order[s];
        if (id < 0 || id >= n) { atomicOr(&hdr[6], kFlagBadOrder); id = 0; }      // not dereferenced; the build is refused
        rows[s] = make_float4(pos[id * 3], pos[id * 3 + 1], pos[id * 3 + 2], 0.f);
    }
}

__device__ __forceinline__ void store_box(float4* __restrict__ nodes, int64_t node, const float* lo, const float* hi) {
    nodes[2 * node] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    nodes[2 * node + 1] = make_float4(hi[1], hi[2], 0.f, 0.f);
}

// leaf slot j -> node L - 1 + j: the box of sorted points [8 j, 8 j + 8), empty past the last point
__global__ __launch_bounds__(256) void cloud_leaves_kernel(const float4* __restrict__ rows, int64_t n, int L, float4* __restrict__ nodes) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < L; j += (int64_t)gridDim.x * blockDim.x) {
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        for (int64_t s = j * kGwSplit; s < n && s < (j + 1) * kGwSplit; ++s) {
            const float4 q = rows[s];
            lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
            hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
        }
        store_box(nodes, (int64_t)L - 1 + j, lo, hi);
    }
}

// nodes [first, first + count) of one level from their children on the level below
__global__ __launch_bounds__(256) void cloud_level_kernel(float4* __restrict__ nodes, int first, int count) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const int64_t n = (int64_t)first + i;
        const float4 a0 = nodes[2 * (2 * n + 1)], a1 = nodes[2 * (2 * n + 1) + 1], b0 = nodes[2 * (2 * n + 2)], b1 = nodes[2 * (2 * n + 2) + 1];
        const float lo[3] = {fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z)};
        const float hi[3] = {fmaxf(a0.w, b0.w), fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y)};
        store_box(nodes, n, lo, hi);
    }
}

// ---- the batch ------------------------------------------------------------------------------------------------------------------------
// Keys, arguments and sample generation: sample_batch_kernel's (dudf_sample.hip), restated.
__host__ __device__ __forceinline__ uint64_t stream_key(uint64_t seed, uint64_t stream) {
    return dudf_splitmix64(seed * 0x100000001B3ull + stream);
}

struct SampleArgs {
    const float *pc_pos, *pc_nrm;
    float *x, *normals, *sdf;
    int64_t n_pc;
    int64_t n_on, n_far, n_near;           // GLOBAL stratum sizes
    int64_t on0, on1, far0, far1, near0, near1;   // this rank's [begin, end) inside each stratum
    uint64_t k_on, k_fx, k_fy, k_fz, k_pick, k_n1, k_n2;
    uint64_t seed; const int64_t* step_dev;         // step_dev != nullptr: the keys are derived in the kernel from (seed, *step_dev)
    unsigned long long* stats;                      // += exact evaluations (may be null)
};

__host__ __device__ __forceinline__ void sample_keys(SampleArgs& a, uint64_t seed, uint64_t step) {
    const uint64_t base = 1000ull * step;
    a.k_on = stream_key(seed, base + 400); a.k_fx = stream_key(seed, base + 401); a.k_fy = stream_key(seed, base + 402);
    a.k_fz = stream_key(seed, base + 403); a.k_pick = stream_key(seed, base + 404);
    a.k_n1 = stream_key(seed, base + 405); a.k_n2 = stream_key(seed, base + 406);
}

// kCloud: the tree holds the cloud's points and only the far stratum is measured (near sdf = |offset|); otherwise it holds the
// mesh's triangles and both off-surface strata are.  Thread -> (sample, lane of its group) as in sample_batch_kernel; a group whose
// sample needs no distance skips the walk, a wave ends when its eight groups have.  No barrier.
template <bool kCloud>
__global__ __launch_bounds__(kGwBlock) void sample_indexed_kernel(SampleArgs a, GwTree t) {
    // no a*b+c -> fma here: see sample_batch_kernel (the oracle rounds the product of normal and offset to fp32 before the add)
#pragma clang fp contract(off)
    if (a.step_dev) sample_keys(a, a.seed, (uint64_t)*a.step_dev);     // graph replay: this launch's step lives in device memory
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int group = threadIdx.x / kGwSplit;
    int* snode = reinterpret_cast<int*>(smem) + group;                                            // [depth][kGwGroups]
    float* slb = reinterpret_cast<float*>(smem) + (size_t)t.depth * kGwGroups + group;            // [depth][kGwGroups]
    const int64_t n_on_l = a.on1 - a.on0, n_far_l = a.far1 - a.far0, n_near_l = a.near1 - a.near0;
    const int64_t n_l = n_on_l + n_far_l + n_near_l;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid / kGwSplit;
    const int part = (int)(gid % kGwSplit);
    const bool live = i < n_l;
    float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, known = 0.f;
    bool query = false;
    if (live) {
        if (i < n_on_l) {
            const int64_t g = a.on0 + i;
            const int64_t c = (int64_t)(dudf_uniform01(a.k_on, (uint64_t)g) * (double)a.n_pc);
            px = a.pc_pos[c * 3]; py = a.pc_pos[c * 3 + 1]; pz = a.pc_pos[c * 3 + 2];
            nx = a.pc_nrm[c * 3]; ny = a.pc_nrm[c * 3 + 1]; nz = a.pc_nrm[c * 3 + 2];
        } else if (i < n_on_l + n_far_l) {
            const uint64_t g = (uint64_t)(a.far0 + (i - n_on_l));
            px = (float)(dudf_uniform01(a.k_fx, g) * 2.0 - 1.0);
            py = (float)(dudf_uniform01(a.k_fy, g) * 2.0 - 1.0);
            pz = (float)(dudf_uniform01(a.k_fz, g) * 2.0 - 1.0);
            query = true;
        } else {
            const uint64_t g = (uint64_t)(a.near0 + (i - n_on_l - n_far_l));
            const int64_t k = (int64_t)(dudf_uniform01(a.k_pick, g) * (double)a.n_on);       // which on-surface sample
            const int64_t c = (int64_t)(dudf_uniform01(a.k_on, (uint64_t)k) * (double)a.n_pc);
            const double u1 = dudf_uniform01(a.k_n1, g), u2 = dudf_uniform01(a.k_n2, g);
            const float off = (float)(0.01 * sqrt(-2.0 * log1p(-u1)) * cos(6.283185307179586476925 * u2));
            px = __fadd_rn(a.pc_pos[c * 3], __fmul_rn(a.pc_nrm[c * 3], off));
            py = __fadd_rn(a.pc_pos[c * 3 + 1], __fmul_rn(a.pc_nrm[c * 3 + 1], off));
            pz = __fadd_rn(a.pc_pos[c * 3 + 2], __fmul_rn(a.pc_nrm[c * 3 + 2], off));
            query = !kCloud;
            known = fabsf(off);
        }
    }
    double best = 3.0e38;                                             // where sample_batch_kernel's scan starts
    unsigned long long evals = 0;
    if (query) best = gw_walk_nearest<typename std::conditional<kCloud, GwPointLeaf, GwTriLeaf>::type>(t, snode, slb, px, py, pz, part, best, evals);
    if (a.stats) {                                                    // one atomic per wave; integer: order does not matter
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) evals += __shfl_xor(evals, m);
        if ((threadIdx.x & 63) == 0 && evals) atomicAdd(a.stats, evals);
    }
    if (live && part == 0) {
        a.x[i * 3] = px; a.x[i * 3 + 1] = py; a.x[i * 3 + 2] = pz;
        a.normals[i * 3] = nx; a.normals[i * 3 + 1] = ny; a.normals[i * 3 + 2] = nz;
        // off-surface samples keep sdf > 0, as in sample_batch_kernel (sdf == 0 marks "on surface" for the loss kernels)
        const float sd = query ? (float)sqrt(best) : known;
        a.sdf[i] = (i < n_on_l) ? sd : fmaxf(sd, 1.17549435e-38f);
    }
}

// an index the call needs: (NULL, 0) = the caller has none (DUDF_E_BADCFG); otherwise there, aligned and of exactly `need` bytes
int check_index(const void* index, size_t index_bytes, size_t need) {
    if (!index && index_bytes == 0) return DUDF_E_BADCFG;
    if (index_bytes != need) return DUDF_E_WORKSPACE;
    return dudf_check_buffer(index, index_bytes, need);
}

int sample_indexed_impl(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc, int64_t n_on,
                        int64_t n_far, int64_t n_near, uint64_t seed, uint64_t step, const int64_t* step_dev, int rank, int world,
                        const void* mesh_index, size_t mesh_index_bytes, const void* cloud_index, size_t cloud_index_bytes,
                        float* x, float* normals, float* sdf, int64_t* out_stats, void* stream) {
    if (n_tri < 0 || (n_tri > 0 && !tri) || n_pc <= 0 || world < 1 || rank < 0 || rank >= world || n_on < 0 || n_far < 0 || n_near < 0)
        return DUDF_E_BADCFG;
    if (n_near > 0 && n_on == 0) return DUDF_E_BADCFG;
    if (n_tri >= ((int64_t)1 << 31) || (n_tri == 0 && n_pc >= ((int64_t)1 << 31))) return DUDF_E_UNSUPPORTED;
    const bool cloud = n_tri == 0;
    GwTree t;
    if (cloud) {
        const GwCloudLayout y = gw_carve_cloud(cloud_index, n_pc);
        if (int rc = check_index(cloud_index, cloud_index_bytes, y.total)) return rc;
        t.nodes = y.nodes; t.prims = y.rows; t.n = n_pc; t.L = y.L; t.depth = y.depth;
    } else {
        const GwMeshLayout y = gw_carve_mesh(mesh_index, n_tri);
        if (int rc = check_index(mesh_index, mesh_index_bytes, y.total)) return rc;
        t.nodes = y.nodes; t.prims = y.stri; t.n = n_tri; t.L = y.L; t.depth = y.depth;
    }
    SampleArgs a;
    a.pc_pos = pc_pos; a.pc_nrm = pc_nrm; a.x = x; a.normals = normals; a.sdf = sdf;
    a.n_pc = n_pc; a.n_on = n_on; a.n_far = n_far; a.n_near = n_near;
    auto lo = [&](int64_t m) { return m * rank / world; };
    auto hi = [&](int64_t m) { return m * (rank + 1) / world; };
    a.on0 = lo(n_on); a.on1 = hi(n_on); a.far0 = lo(n_far); a.far1 = hi(n_far); a.near0 = lo(n_near); a.near1 = hi(n_near);
    a.seed = seed; a.step_dev = step_dev; a.stats = reinterpret_cast<unsigned long long*>(out_stats);
    sample_keys(a, seed, step);
    const int64_t n_l = (a.on1 - a.on0) + (a.far1 - a.far0) + (a.near1 - a.near0);
    if (n_l == 0) return 0;
    const int64_t blocks = (n_l * kGwSplit + kGwBlock - 1) / kGwBlock;
    if (blocks >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const dim3 grid((unsigned)blocks);
    if (cloud) return dudf_launch_lds(sample_indexed_kernel<true>, grid, dim3(kGwBlock), gw_lds_bytes(t), st, a, t);
    return dudf_launch_lds(sample_indexed_kernel<false>, grid, dim3(kGwBlock), gw_lds_bytes(t), st, a, t);
}

// header: bounds of all points and the non-finite flag; clears the other flags
int launch_bounds(const float* pos, int64_t n, unsigned* hdr, hipStream_t st) {
    DUDF_TRY(hipMemsetAsync(hdr, 0, kGwHdrBytes, st));                        // max words 0 (below every encoded float), flags 0
    DUDF_TRY(hipMemsetAsync(hdr, 0xff, 3 * sizeof(unsigned), st));            // min words above every encoded float
    return dudf_launch(cloud_bounds_kernel, dim3(dudf_grid_for(n, 256, 256)), dim3(256), st, pos, n, hdr);
}

}  // namespace

extern "C" {

size_t dudf_cloud_index_bytes(int64_t n_pc) {
    if (n_pc <= 0 || n_pc >= ((int64_t)1 << 31)) return 0;
    return gw_carve_cloud(nullptr, n_pc).total;
}

int dudf_cloud_morton_codes(const float* pc_pos, int64_t n_pc, void* index, size_t index_bytes, int64_t* codes, void* stream) {
    if (n_pc <= 0 || !pc_pos || !codes) return DUDF_E_BADCFG;
    if (n_pc >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (int rc = dudf_check_buffer(index, index_bytes, gw_carve_cloud(nullptr, n_pc).total)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    unsigned* hdr = gw_carve_cloud(index, n_pc).hdr;
    DUDF_TRY(launch_bounds(pc_pos, n_pc, hdr, st));
    return dudf_launch(cloud_codes_kernel, dim3(dudf_grid_for(n_pc, 256, kGridCap)), dim3(256), st, pc_pos, n_pc, hdr, codes);
}

int dudf_cloud_index_build(const float* pc_pos, int64_t n_pc, const int64_t* order, void* index, size_t index_bytes, void* stream) {
    if (n_pc <= 0 || !pc_pos || !order) return DUDF_E_BADCFG;
    if (n_pc >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (int rc = dudf_check_buffer(index, index_bytes, gw_carve_cloud(nullptr, n_pc).total)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const GwCloudLayout y = gw_carve_cloud(index, n_pc);
    DUDF_TRY(launch_bounds(pc_pos, n_pc, y.hdr, st));                         // the build stands alone: any permutation is a valid order
    DUDF_TRY(dudf_launch(cloud_gather_kernel, dim3(dudf_grid_for(n_pc, 256, kGridCap)), dim3(256), st, pc_pos, n_pc, order, y.rows, y.hdr));
    DUDF_TRY(dudf_launch(cloud_leaves_kernel, dim3(dudf_grid_for(y.L, 256, kGridCap)), dim3(256), st, y.rows, n_pc, y.L, y.nodes));
    for (int count = y.L / 2; count >= 1; count /= 2)                         // level of `count` nodes starts at node count - 1
        DUDF_TRY(dudf_launch(cloud_level_kernel, dim3(dudf_grid_for(count, 256, kGridCap)), dim3(256), st, y.nodes, count - 1, count));
    return 0;
}

int dudf_sample_batch_indexed(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc, int64_t n_on,
                              int64_t n_far, int64_t n_near, uint64_t seed, uint64_t step, int rank, int world,
                              const void* mesh_index, size_t mesh_index_bytes, const void* cloud_index, size_t cloud_index_bytes,
                              float* x, float* normals, float* sdf, int64_t* out_stats, void* stream) {
    return sample_indexed_impl(tri, n_tri, pc_pos, pc_nrm, n_pc, n_on, n_far, n_near, seed, step, nullptr, rank, world, mesh_index,
                               mesh_index_bytes, cloud_index, cloud_index_bytes, x, normals, sdf, out_stats, stream);
}

int dudf_sample_batch_indexed_at(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc, int64_t n_on,
                                 int64_t n_far, int64_t n_near, uint64_t seed, const int64_t* step_dev, int rank, int world,
                                 const void* mesh_index, size_t mesh_index_bytes, const void* cloud_index, size_t cloud_index_bytes,
                                 float* x, float* normals, float* sdf, int64_t* out_stats, void* stream) {
    if (!step_dev) return DUDF_E_BADCFG;
    return sample_indexed_impl(tri, n_tri, pc_pos, pc_nrm, n_pc, n_on, n_far, n_near, seed, 0, step_dev, rank, world, mesh_index,
                               mesh_index_bytes, cloud_index, cloud_index_bytes, x, normals, sdf, out_stats, stream);
}

}  // extern "C"
