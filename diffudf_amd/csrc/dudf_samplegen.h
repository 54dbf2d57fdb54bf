// The per-step training batch as dudf_sample.hip (a scan of the whole shape) and dudf_sample_indexed.hip (a walk of an index) both
// draw it: keys, sharding, the three strata [on | far | near], the argument checks and the final store, stated once.  What the two
// kernels do between sample_point and sample_store — finding the distance of an off-surface sample — is theirs.  The layout of the
// batch and its reference are described at the head of dudf_sample.hip.  Internal.
#ifndef DUDF_SAMPLEGEN_H
#define DUDF_SAMPLEGEN_H
#include "dudf_internal.h"
#include "dudf_rng.h"              // dudf_splitmix64, dudf_uniform01

__host__ __device__ __forceinline__ uint64_t stream_key(uint64_t seed, uint64_t stream) {
    return dudf_splitmix64(seed * 0x100000001B3ull + stream);
}

struct SampleArgs {
    const float *tri, *pc_pos, *pc_nrm;
    float *x, *normals, *sdf;
    int64_t n_tri, n_pc;
    int64_t n_on, n_far, n_near;           // GLOBAL stratum sizes
    int64_t on0, on1, far0, far1, near0, near1;   // this rank's [begin, end) inside each stratum
    uint64_t k_on, k_fx, k_fy, k_fz, k_pick, k_n1, k_n2;
    uint64_t seed; const int64_t* step_dev;         // step_dev != nullptr: the keys are derived in the kernel from (seed, *step_dev)
};

__host__ __device__ __forceinline__ void sample_keys(SampleArgs& a, uint64_t seed, uint64_t step) {
    const uint64_t base = 1000ull * step;
    a.k_on = stream_key(seed, base + 400); a.k_fx = stream_key(seed, base + 401); a.k_fy = stream_key(seed, base + 402);
    a.k_fz = stream_key(seed, base + 403); a.k_pick = stream_key(seed, base + 404);
    a.k_n1 = stream_key(seed, base + 405); a.k_n2 = stream_key(seed, base + 406);
}

// samples of this rank
inline int64_t sample_count(const SampleArgs& a) { return (a.on1 - a.on0) + (a.far1 - a.far0) + (a.near1 - a.near0); }

// The refusals every batch entry point makes first, then `a` from its arguments: rank `rank` of `world` takes [m r / W, m (r + 1) / W)
// of each stratum of m.  No device call.
inline int sample_args(SampleArgs& a, const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc, int64_t n_on,
                       int64_t n_far, int64_t n_near, uint64_t seed, uint64_t step, const int64_t* step_dev, int rank, int world, float* x,
                       float* normals, float* sdf) {
    if (n_tri < 0 || (n_tri > 0 && !tri) || n_pc <= 0 || world < 1 || rank < 0 || rank >= world || n_on < 0 || n_far < 0 || n_near < 0)
        return DUDF_E_BADCFG;
    if (n_near > 0 && n_on == 0) return DUDF_E_BADCFG;
    a.tri = tri; a.pc_pos = pc_pos; a.pc_nrm = pc_nrm; a.x = x; a.normals = normals; a.sdf = sdf;
    a.n_tri = n_tri; a.n_pc = n_pc; a.n_on = n_on; a.n_far = n_far; a.n_near = n_near;
    auto lo = [&](int64_t m) { return m * rank / world; };
    auto hi = [&](int64_t m) { return m * (rank + 1) / world; };
    a.on0 = lo(n_on); a.on1 = hi(n_on); a.far0 = lo(n_far); a.far1 = hi(n_far); a.near0 = lo(n_near); a.near1 = hi(n_near);
    a.seed = seed; a.step_dev = step_dev;
    sample_keys(a, seed, step);
    return 0;
}

// Local sample i of the batch, n_on_l / n_far_l = this rank's on-surface / far samples: its position p and its normal n (on-surface
// samples only).  Returns whether its sdf is a distance still to be measured; otherwise the sdf is `known`.  cloud: a
// point-cloud-only shape, whose near samples carry |offset| instead of a distance.
__device__ __forceinline__ bool sample_point(const SampleArgs& a, int64_t i, int64_t n_on_l, int64_t n_far_l, bool cloud, float& px,
                                             float& py, float& pz, float& nx, float& ny, float& nz, float& known) {
    // no a*b+c -> fma here: the oracle (numpy) rounds the product of normal and offset to fp32 before the add, and HIP's
    // __fmul_rn / __fadd_rn are plain operators that hipcc's default -ffp-contract=fast would fuse (measured: 48 of 999
    // near points off by one ulp)
#pragma clang fp contract(off)
    bool query = false;
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
        query = !cloud;
        known = fabsf(off);
    }
    return query;
}

// ... and its row of the batch, `best` the squared distance of a sample whose sdf had to be measured (`query`).
// off-surface samples keep sdf > 0: a far point that lies exactly on a triangle, or a near point whose offset rounds to 0, would
// otherwise carry the "on surface" marker (sdf == 0) in the wrong stratum — the loss kernels' n_hess layout check turns that
// into NaN for the rest of the run.  FLT_MIN as a distance is 0 to every later computation.
__device__ __forceinline__ void sample_store(const SampleArgs& a, int64_t i, int64_t n_on_l, float px, float py, float pz, float nx, float ny,
                                             float nz, bool query, double best, float known) {
    a.x[i * 3] = px; a.x[i * 3 + 1] = py; a.x[i * 3 + 2] = pz;
    a.normals[i * 3] = nx; a.normals[i * 3 + 1] = ny; a.normals[i * 3 + 2] = nz;
    const float sd = query ? (float)sqrt(best) : known;
    a.sdf[i] = (i < n_on_l) ? sd : fmaxf(sd, 1.17549435e-38f);
}

#endif  // DUDF_SAMPLEGEN_H
