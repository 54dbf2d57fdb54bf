// Surface-sampled evaluation on the device: an area-uniform sampler of a triangle mesh and the threshold statistics of a distance
// vector — what `diffudf_amd.metrics.surface_metrics` (Chamfer distance on surface samples, F-score, Hausdorff) is made of.  Kernels
// and their C entry points (include/dudf_hip.h); the rules are DESIGN.md §8 and tests/surface_oracle.py restates them in numpy.
// Built without contraction (Makefile): the double arithmetic below is the oracle's, product by product.
//
// The sampler picks faces by INTEGER weights.  A cumulative sum of double areas depends on the order of its additions, so a scan on
// the device could not give the bits of any host sum, nor the same bits for two launch geometries.  Here
//   nn_f = |e1 x e2| in fp64, nn_max = max_f nn_f (an integer atomicMax on the bits: order-free),
//   w_f = floor(nn_f / nn_max * 2^32) (one correctly rounded division, one exact scaling), c_f = w_0 + .. + w_f in uint64,
// and integer sums are exact in every order: W = c_{F-1} < 2^31 * 2^32.  A sample's 53 random bits k choose
// t = floor(k W / 2^53) in [0, W) and the face is the first f with c_f > t — `searchsorted(c, t, side="right")`.  A face of weight 0
// repeats its predecessor's c and is never the first.
#include "dudf_context.h"
#include "dudf_ordsum.h"
#include "dudf_rng.h"
#include "dudf_wgscan.h"
#include <string.h>

namespace {

static_assert(DUDF_WG == kOrdSumBlock, "the face sum's launch is sized by dudf_ordsum_groups");
constexpr int kGridCap = 4096;                   // workgroups of the row-wise launches; the kernels stride over the rest
constexpr unsigned kFlagNonFinite = 1u, kFlagBadIndex = 2u;
constexpr double kTwo32 = 4294967296.0, kTwo53 = 9007199254740992.0;
constexpr int kStatsMaxK = 16;

struct SampleStatus {                            // one granule of the workspace; the host reads it once per call
    unsigned long long max_bits;                 // bits of nn_max (non-negative doubles order like their bits)
    uint64_t total;                              // W
    unsigned flags;
    unsigned pad;
};

// ---- faces: normal, |e1 x e2|, area partials, maximum ---------------------------------------------------------------------------
// The area partials are an ordered sum (dudf_ordsum.h), the maximum rides the same tree: partials[b] is a function of (F, inputs,
// gridDim) only, and gridDim is a function of F.
__global__ __launch_bounds__(DUDF_WG) void surf_faces_kernel(const double* __restrict__ v, int64_t nv, const int64_t* __restrict__ f,
                                                             int64_t nf, double* __restrict__ nn_out, float* __restrict__ fn_out,
                                                             double* __restrict__ partials, SampleStatus* __restrict__ status) {
    __shared__ double sa[DUDF_WG];
    __shared__ unsigned long long sm[DUDF_WG];
    double a = 0.0;
    unsigned long long mx = 0;
    unsigned flags = 0;
    for (int64_t t = (int64_t)blockIdx.x * DUDF_WG + threadIdx.x; t < nf; t += (int64_t)gridDim.x * DUDF_WG) {
        const int64_t i0 = f[t * 3], i1 = f[t * 3 + 1], i2 = f[t * 3 + 2];
        double n0 = 0.0, n1 = 0.0, n2 = 0.0, nn = 0.0;
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
            flags |= kFlagBadIndex;              // not dereferenced; the call fails
        } else {
            const double e0 = v[i1 * 3] - v[i0 * 3], e1 = v[i1 * 3 + 1] - v[i0 * 3 + 1], e2 = v[i1 * 3 + 2] - v[i0 * 3 + 2];
            const double g0 = v[i2 * 3] - v[i0 * 3], g1 = v[i2 * 3 + 1] - v[i0 * 3 + 1], g2 = v[i2 * 3 + 2] - v[i0 * 3 + 2];
            n0 = e1 * g2 - e2 * g1; n1 = e2 * g0 - e0 * g2; n2 = e0 * g1 - e1 * g0;
            nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            if (!(nn <= 1.79769313486231570815e308)) { flags |= kFlagNonFinite; nn = 0.0; n0 = n1 = n2 = 0.0; }
        }
        const double den = nn > 1e-300 ? nn : 1e-300;
        nn_out[t] = nn;
        fn_out[t * 3] = (float)(n0 / den); fn_out[t * 3 + 1] = (float)(n1 / den); fn_out[t * 3 + 2] = (float)(n2 / den);
        a += nn;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(nn);
        mx = bits > mx ? bits : mx;
    }
    sa[threadIdx.x] = a; sm[threadIdx.x] = mx;
    dudf_wg_tree<DUDF_WG>(dudf_sum_of(sa), dudf_max_of(sm));
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sa[0];
        atomicMax(&status->max_bits, sm[0]);
    }
    if (flags) atomicOr(&status->flags, flags);
}

__global__ __launch_bounds__(kOrdSumMaxGroups) void surf_area_kernel(const double* __restrict__ partials, int count,
                                                                     double* __restrict__ out_area) {
    double a[1];
    dudf_ordsum_finish(partials, count, a);
    if (threadIdx.x == 0) *out_area = 0.5 * a[0];
}

// ---- integer weights and their inclusive sums -------------------------------------------------------------------------------------
// one workgroup per DUDF_WG faces: c[f] = the inclusive sum inside the workgroup, blk[b] = the workgroup's total
__global__ __launch_bounds__(DUDF_WG) void surf_weights_kernel(const double* __restrict__ nn, int64_t nf, double nn_max,
                                                               unsigned long long* __restrict__ c, uint64_t* __restrict__ blk) {
    __shared__ unsigned long long wave_tot[DUDF_WG / 64];
    const int64_t t = (int64_t)blockIdx.x * DUDF_WG + threadIdx.x;
    unsigned long long w = 0;
    if (t < nf) w = (unsigned long long)floor(nn[t] / nn_max * kTwo32);    // nn <= nn_max: at most 2^32
    unsigned long long total;
    const unsigned long long before = dudf_wg_scan64(w, wave_tot, &total);
    if (t < nf) c[t] = before + w;
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(DUDF_WG) void surf_offsets_kernel(unsigned long long* __restrict__ c, int64_t nf,
                                                               const uint64_t* __restrict__ off) {
    for (int64_t t = (int64_t)blockIdx.x * DUDF_WG + threadIdx.x; t < nf; t += (int64_t)gridDim.x * DUDF_WG) c[t] += off[t / DUDF_WG];
}

// ---- samples ------------------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    const double* v; const int64_t* f; int64_t nf;
    const unsigned long long* c; const float* fn;
    int64_t start, n;
    uint64_t k1, k2, k3;
    const double* uniforms;
    float* out_points; float* out_normals; int64_t* out_face;
};

__device__ __forceinline__ uint64_t surf_bits(uint64_t key, uint64_t idx) { return dudf_splitmix64(dudf_splitmix64(idx ^ key) + key); }

// One sample per thread: a pure function of (mesh, seed, start + i).  The search is log2 F dependent loads from c, which stays in L2.
__global__ __launch_bounds__(DUDF_WG) void surf_sample_kernel(SampleArgs a) {
    const unsigned long long W = a.c[a.nf - 1];
    for (int64_t i = (int64_t)blockIdx.x * DUDF_WG + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * DUDF_WG) {
        unsigned long long kbits;                                           // k * 2^11, k = u1 * 2^53 an integer below 2^53
        double r1, r2;
        bool ok = true;
        if (a.uniforms) {
            const double u1 = a.uniforms[i * 3];
            r1 = a.uniforms[i * 3 + 1]; r2 = a.uniforms[i * 3 + 2];
            ok = u1 >= 0.0 && u1 < 1.0 && r1 >= 0.0 && r1 < 1.0 && r2 >= 0.0 && r2 < 1.0;      // false for NaN
            kbits = ok ? (unsigned long long)floor(u1 * kTwo53) << 11 : 0;
        } else {
            const uint64_t g = (uint64_t)(a.start + i);
            kbits = surf_bits(a.k1, g) & ~0x7FFull;
            r1 = (double)(surf_bits(a.k2, g) >> 11) * (1.0 / kTwo53);
            r2 = (double)(surf_bits(a.k3, g) >> 11) * (1.0 / kTwo53);
        }
        const unsigned long long t = __umul64hi(kbits, W);                  // floor(k W / 2^53) < W
        int64_t lo = 0, hi = a.nf - 1;                                      // the first f with c[f] > t; c[nf - 1] = W > t
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.c[mid] > t) hi = mid; else lo = mid + 1;
        }
        const int64_t i0 = a.f[lo * 3], i1 = a.f[lo * 3 + 1], i2 = a.f[lo * 3 + 2];   // in range: surf_faces_kernel looked
        const double s = sqrt(r1);
        const double wa = 1.0 - s, wb = s * (1.0 - r2), wc = s * r2;
        float p[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = (float)((wa * a.v[i0 * 3 + q] + wb * a.v[i1 * 3 + q]) + wc * a.v[i2 * 3 + q]);
        const float nanf_ = __builtin_nanf("");
        a.out_points[i * 3] = ok ? p[0] : nanf_; a.out_points[i * 3 + 1] = ok ? p[1] : nanf_; a.out_points[i * 3 + 2] = ok ? p[2] : nanf_;
        if (a.out_normals) {
            a.out_normals[i * 3] = a.fn[lo * 3]; a.out_normals[i * 3 + 1] = a.fn[lo * 3 + 1]; a.out_normals[i * 3 + 2] = a.fn[lo * 3 + 2];
        }
        if (a.out_face) a.out_face[i] = ok ? lo : -1;
    }
}

struct SampleCarve {
    SampleStatus* status; double* partials; double* nn; float* fn; unsigned long long* c; uint64_t* blk; uint64_t* off;
    size_t bytes;
};
inline SampleCarve carve_sample(const void* base, int64_t F) {
    DudfByteCarver cv = dudf_carve(base);
    SampleCarve s;
    const int64_t nblocks = (F + DUDF_WG - 1) / DUDF_WG;
    s.status = cv.take<SampleStatus>(1);
    s.partials = cv.take<double>(kOrdSumMaxGroups);
    s.nn = cv.take<double>(F);
    s.fn = cv.take<float>(F * 3);
    s.c = cv.take<unsigned long long>(F);
    s.blk = cv.take<uint64_t>(nblocks);
    s.off = cv.take<uint64_t>(nblocks);
    s.bytes = cv.o;
    return s;
}

// ---- threshold statistics -----------------------------------------------------------------------------------------------------------
struct StatsTaus { double tau[kStatsMaxK]; };

// Counts and the maximum are integers: atomics in any order give the same words.  The two double sums are ordered sums (dudf_ordsum.h).
__global__ __launch_bounds__(kOrdSumBlock) void stats_partial_kernel(const float* __restrict__ dist, int64_t n, StatsTaus taus, int K,
                                                                     unsigned long long* __restrict__ out_counts,
                                                                     unsigned* __restrict__ out_max, double* __restrict__ partials) {
    __shared__ unsigned long long scnt[kStatsMaxK + 1];
    __shared__ unsigned smax;
    if (threadIdx.x <= kStatsMaxK) scnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    unsigned long long cnt[kStatsMaxK + 1] = {};
    unsigned mx = 0;
    double a = 0.0, b = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kOrdSumBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kOrdSumBlock) {
        const float df = dist[p];
        if (df != df) { cnt[kStatsMaxK] += 1; continue; }
        const double d = (double)df;
#pragma unroll
        for (int k = 0; k < kStatsMaxK; ++k) cnt[k] += (k < K && d <= taus.tau[k]) ? 1u : 0u;
        const unsigned bits = df > 0.0f ? __float_as_uint(df) : 0u;        // distances are non-negative; -0 and below count as 0
        mx = bits > mx ? bits : mx;
        a += d; b += d * d;
    }
#pragma unroll
    for (int k = 0; k <= kStatsMaxK; ++k) {
        unsigned long long c = cnt[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&scnt[k], c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned other = __shfl_down(mx, o); mx = other > mx ? other : mx; }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&smax, mx);
    const double sums[2] = {a, b};
    dudf_ordsum_partial<kOrdSumBlock>(sums, partials);          // its barriers also close the atomics on scnt and smax
    if (threadIdx.x == 0 && smax) atomicMax(out_max, smax);
    if ((int)threadIdx.x < K && scnt[threadIdx.x]) atomicAdd(&out_counts[threadIdx.x], scnt[threadIdx.x]);
    if (threadIdx.x == kStatsMaxK && scnt[kStatsMaxK]) atomicAdd(&out_counts[K], scnt[kStatsMaxK]);
}

__global__ __launch_bounds__(kOrdSumMaxGroups) void stats_final_kernel(const double* __restrict__ partials, int count,
                                                                       double* __restrict__ out_sums) {
    double sums[2];
    dudf_ordsum_finish(partials, count, sums);
    if (threadIdx.x == 0) { out_sums[0] = sums[0]; out_sums[1] = sums[1]; }
}

}  // namespace

extern "C" {

size_t dudf_mesh_sample_surface_workspace(int64_t F) {
    if (F <= 0 || F >= ((int64_t)1 << 31)) return 0;
    return carve_sample(nullptr, F).bytes;
}

int dudf_mesh_sample_surface(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int64_t start, int64_t n,
                             uint64_t seed, const double* uniforms, float* out_points, float* out_normals, int64_t* out_face,
                             float* out_face_normals, double* out_area, void* workspace, size_t workspace_bytes, void* stream) {
    if (F <= 0 || V <= 0 || n < 0 || start < 0 || !vertices || !faces || (n > 0 && !out_points)) return DUDF_E_BADCFG;
    if (F >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (start > INT64_MAX - n) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_mesh_sample_surface_workspace(F))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const SampleCarve w = carve_sample(workspace, F);
    float* fn = out_face_normals ? out_face_normals : w.fn;
    DUDF_TRY(hipMemsetAsync(w.status, 0, sizeof(SampleStatus), st));
    const int groups = dudf_ordsum_groups(F);
    DUDF_TRY(dudf_launch(surf_faces_kernel, dim3(groups), dim3(DUDF_WG), st, vertices, V, faces, F, w.nn, fn, w.partials, w.status));
    if (out_area) DUDF_TRY(dudf_launch(surf_area_kernel, dim3(1), dim3(kOrdSumMaxGroups), st, w.partials, groups, out_area));
    // the one host read of the call: the weights need nn_max, and a mesh without area or with a bad face is refused here
    SampleStatus h;
    DUDF_TRY(hipMemcpyAsync(&h, w.status, sizeof(SampleStatus), hipMemcpyDeviceToHost, st));
    DUDF_TRY(hipStreamSynchronize(st));
    if (h.flags & (kFlagBadIndex | kFlagNonFinite)) return DUDF_E_BADMODE;
    double nn_max;
    memcpy(&nn_max, &h.max_bits, sizeof(double));
    if (!(nn_max > 0.0)) return DUDF_E_BADCFG;
    if (n == 0) return 0;
    const int64_t nblocks = (F + DUDF_WG - 1) / DUDF_WG;
    DUDF_TRY(dudf_launch(surf_weights_kernel, dim3((unsigned)nblocks), dim3(DUDF_WG), st, w.nn, F, nn_max, w.c, w.blk));
    if (nblocks > 1) {
        DUDF_TRY(dudf_launch(dudf_scan_totals64_kernel, dim3(1), dim3(1024), st, w.blk, w.off, nblocks, &w.status->total));
        DUDF_TRY(dudf_launch(surf_offsets_kernel, dim3(dudf_grid_for(F, DUDF_WG, kGridCap)), dim3(DUDF_WG), st, w.c, F, w.off));
    }
    SampleArgs a;
    a.v = vertices; a.f = faces; a.nf = F; a.c = w.c; a.fn = fn; a.start = start; a.n = n;
    a.k1 = dudf_splitmix64(seed * 0x100000001B3ull + 301); a.k2 = dudf_splitmix64(seed * 0x100000001B3ull + 302);
    a.k3 = dudf_splitmix64(seed * 0x100000001B3ull + 303);
    a.uniforms = uniforms; a.out_points = out_points; a.out_normals = out_normals; a.out_face = out_face;
    return dudf_launch(surf_sample_kernel, dim3(dudf_grid_for(n, DUDF_WG, kGridCap)), dim3(DUDF_WG), st, a);
}

size_t dudf_distance_stats_workspace_bytes(int64_t n) { return dudf_round256((size_t)dudf_ordsum_groups(n) * 2 * sizeof(double)); }   // >= 256

int dudf_distance_stats(const float* dist, int64_t n, const double* thresholds, int K, int64_t* out_counts, float* out_max,
                        double* out_sums, void* workspace, size_t workspace_bytes, void* stream) {
    if (K < 0 || K > kStatsMaxK) return DUDF_E_UNSUPPORTED;
    if (n < 0 || !out_counts || !out_max || !out_sums || (n > 0 && !dist) || (K > 0 && !thresholds)) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_distance_stats_workspace_bytes(n))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    double* partials = reinterpret_cast<double*>(workspace);
    StatsTaus taus = {};
    for (int k = 0; k < K; ++k) taus.tau[k] = thresholds[k];
    DUDF_TRY(hipMemsetAsync(out_counts, 0, (size_t)(K + 1) * sizeof(int64_t), st));
    DUDF_TRY(hipMemsetAsync(out_max, 0, sizeof(float), st));
    const int groups = n > 0 ? dudf_ordsum_groups(n) : 0;
    if (groups > 0)
        DUDF_TRY(dudf_launch(stats_partial_kernel, dim3(groups), dim3(kOrdSumBlock), st, dist, n, taus, K,
                             reinterpret_cast<unsigned long long*>(out_counts), reinterpret_cast<unsigned*>(out_max), partials));
    return dudf_launch(stats_final_kernel, dim3(1), dim3(kOrdSumMaxGroups), st, partials, groups, out_sums);
}

}  // extern "C"
