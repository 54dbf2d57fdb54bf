// The per-step training batch of dudf_sample.hip with its distances taken through an index instead of a scan of the whole shape —
// for meshes and clouds too large for the scan (its cost per step is linear in the triangles / points; the walk's is logarithmic).
// Kernel and its C entry points (include/dudf_hip.h).
//
//   - mesh input: the off-surface samples walk the mesh index (dudf_bvh.h: leaves of 8 sorted triangles);
//   - cloud input (n_tri == 0): the far samples walk the cloud index over pc_pos (leaves of 8 points as 16-byte rows).
// The walk is dudf_groupwalk.h: 8 lanes per sample, a leaf per step.  The samples are dudf_samplegen.h's, as in sample_batch_kernel,
// and every distance is the minimum of the same exact fp64 values, so the batch is bit-identical to dudf_sample_batch's
// (tests/test_sampler_indexed_gpu.py).  The launch makes no allocation, copy or synchronisation: it can be captured in a graph.
#include "dudf_groupwalk.h"

#include <type_traits>

#include "dudf_samplegen.h"

namespace {

// kCloud: the tree holds the cloud's points and only the far stratum is measured (near sdf = |offset|); otherwise it holds the
// mesh's triangles and both off-surface strata are.  Thread -> (sample, lane of its group) as in sample_batch_kernel; a group whose
// sample needs no distance skips the walk, a wave ends when its eight groups have.  No barrier.  stats += exact evaluations (may be null).
template <bool kCloud>
__global__ __launch_bounds__(kGwBlock) void sample_indexed_kernel(SampleArgs a, GwTree t, unsigned long long* stats) {
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
    if (live) query = sample_point(a, i, n_on_l, n_far_l, kCloud, px, py, pz, nx, ny, nz, known);
    double best = 3.0e38;                                             // where sample_batch_kernel's scan starts
    unsigned long long evals = 0;
    if (query) best = gw_walk_nearest<typename std::conditional<kCloud, GwPointLeaf, GwTriLeaf>::type>(t, snode, slb, px, py, pz, part, best, evals);
    if (stats) {                                                      // one atomic per wave; integer: order does not matter
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) evals += __shfl_xor(evals, m);
        if ((threadIdx.x & 63) == 0 && evals) atomicAdd(stats, evals);
    }
    if (live && part == 0) sample_store(a, i, n_on_l, px, py, pz, nx, ny, nz, query, best, known);
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
    SampleArgs a;
    if (int rc = sample_args(a, tri, n_tri, pc_pos, pc_nrm, n_pc, n_on, n_far, n_near, seed, step, step_dev, rank, world, x, normals, sdf)) return rc;
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
    const int64_t n_l = sample_count(a);
    if (n_l == 0) return 0;
    const int64_t blocks = (n_l * kGwSplit + kGwBlock - 1) / kGwBlock;
    if (blocks >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(out_stats);
    const dim3 grid((unsigned)blocks);
    if (cloud) return dudf_launch_lds(sample_indexed_kernel<true>, grid, dim3(kGwBlock), gw_lds_bytes(t), st, a, t, stats);
    return dudf_launch_lds(sample_indexed_kernel<false>, grid, dim3(kGwBlock), gw_lds_bytes(t), st, a, t, stats);
}

}  // namespace

extern "C" {

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
