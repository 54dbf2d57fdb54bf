// Chamfer distance and normal consistency on the device — what `pytorch3d.loss.chamfer_distance` does for reference
// cuantitative.py:10-19 (`knn_points(x, y, norm, K=1)`, the `abs_cosine` normal term, the sums behind its mean reductions) and
// what open3d's `compute_vertex_normals(normalized=True)` does at :99-100.  Kernels and their C entry points (include/dudf_hip.h).
//
// Nearest neighbour: brute force on DIRECT differences, (x - y) then square or abs, in fp32.  The matmul form |x|^2 + |y|^2 - 2 x.y
// cancels: nearest squared distances of a dense cloud are ~1e-5 against coordinates of ~0.5, which leaves one significant digit.
//   - a lane keeps kNnPpl rows of x in registers; a workgroup covers kNnRows of them;
//   - a tile of y sits in LDS as float4 and is read at a wave-uniform address: one broadcast ds_read_b128 serves 64 * kNnPpl pairs;
//   - n = 1e5 rows are only ~100 workgroups, so the y range is split across blockIdx.y as well, and the per-row results are merged
//     through one uint64 key per row, (float bits of the distance << 32) | index, with a vector 64-bit atomicMin.  Distances are
//     non-negative (a NaN's bits sort above +inf's), so unsigned order of the keys is (distance, index) order: among equal
//     distances the smallest index wins, whatever the launch geometry or the order in which workgroups arrive;
//   - a finishing kernel unpacks the keys.
// Every pair is evaluated by the same expression, so the result is a pure function of the inputs: repeated calls are bit-identical.
#include "dudf_context.h"
#include "dudf_ordsum.h"
#include "dudf_pairdist.h"

namespace {

constexpr int kNnBlock = 256;                    // threads per workgroup
constexpr int kNnPpl = 4;                        // rows of x per lane
constexpr int kNnRows = kNnBlock * kNnPpl;       // rows of x per workgroup
constexpr int kNnTile = 1024;                    // rows of y per LDS tile (16 KiB)
constexpr int kNnTargetGroups = 4096;            // workgroups a launch aims for: two resident rounds of 8 per CU
constexpr unsigned kNanBits = 0x7fc00000u;
constexpr int kGridCap = 4096;                   // workgroups of the row-wise launches; the kernels stride over the rest

// pair_distance<NORM>: dudf_pairdist.h (shared with the K-nearest search of dudf_orient.hip, which must return the same bits)

// grid (ceil(n / kNnRows), splits); workgroup (bx, by) scans y rows [by * ychunk, min(m, (by + 1) * ychunk)) — never empty — for x
// rows bx * kNnRows + k * kNnBlock + lane.  Rows past n repeat row n - 1 and are not written.
template <int NORM>
__global__ __launch_bounds__(kNnBlock) void nearest_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ y, int m,
                                                           int ychunk, unsigned long long* __restrict__ keys) {
    __shared__ float4 tile[kNnTile];
    const int64_t row0 = (int64_t)blockIdx.x * kNnRows + threadIdx.x;
    const int y0 = blockIdx.y * ychunk;
    const int y1 = (m - y0 < ychunk) ? m : y0 + ychunk;
    float ax[kNnPpl], ay[kNnPpl], az[kNnPpl], best[kNnPpl];
    int bi[kNnPpl];
#pragma unroll
    for (int k = 0; k < kNnPpl; ++k) {
        int64_t r = row0 + (int64_t)k * kNnBlock;
        if (r > n - 1) r = n - 1;
        ax[k] = x[r * 3]; ay[k] = x[r * 3 + 1]; az[k] = x[r * 3 + 2];
        best[k] = __builtin_inff();
        bi[k] = y0;                      // in range even if no candidate ever compares below +inf (NaN / overflowing rows)
    }
    for (int t0 = y0; t0 < y1; t0 = (y1 - t0 > kNnTile) ? t0 + kNnTile : y1) {       // (no step past y1: m may be close to 2^31)
        const int cnt = (y1 - t0 < kNnTile) ? y1 - t0 : kNnTile;
        __syncthreads();                 // the previous tile has been read by every wave
        for (int j = threadIdx.x; j < cnt; j += kNnBlock) {
            const float* q = y + (int64_t)(t0 + j) * 3;
            tile[j] = make_float4(q[0], q[1], q[2], 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 q = tile[j];    // wave-uniform address: a broadcast read
#pragma unroll
            for (int k = 0; k < kNnPpl; ++k) {
                const float d = pair_distance<NORM>(ax[k], ay[k], az[k], q);
                if (d < best[k]) { best[k] = d; bi[k] = t0 + j; }       // ascending j, strict <: the smallest index of a tie stays
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kNnPpl; ++k) {
        const int64_t r = row0 + (int64_t)k * kNnBlock;
        if (r >= n) continue;
        unsigned bits = __float_as_uint(best[k]);
        if (ax[k] != ax[k] || ay[k] != ay[k] || az[k] != az[k]) bits = kNanBits;   // a NaN row: NaN distance, index of the first split
        atomicMin(&keys[r], ((unsigned long long)bits << 32) | (unsigned)bi[k]);
    }
}

__global__ __launch_bounds__(256) void nearest_finish_kernel(const unsigned long long* __restrict__ keys, int64_t n, int m,
                                                             float* __restrict__ out_dist, int64_t* __restrict__ out_idx) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[p];
        if (out_dist) out_dist[p] = __uint_as_float((unsigned)(key >> 32));
        if (out_idx) {
            const unsigned j = (unsigned)key;
            out_idx[p] = j < (unsigned)m ? (int64_t)j : 0;     // every key was written by a workgroup with an index in [0, m)
        }
    }
}

// ---- sums behind the mean reductions --------------------------------------------------------------------------------------------
// Two doubles per workgroup: sum of dist and sum of 1 - |cos(x normal, normal of the nearest y row)|, as ordered sums (dudf_ordsum.h):
// a function of (n, inputs) only.
__global__ __launch_bounds__(kOrdSumBlock) void chamfer_partial_kernel(const float* __restrict__ dist, const int64_t* __restrict__ idx,
                                                                       int64_t n, const float* __restrict__ xn,
                                                                       const float* __restrict__ yn, int64_t m,
                                                                       double* __restrict__ partials) {
    double a = 0.0, b = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kOrdSumBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kOrdSumBlock) {
        a += (double)dist[p];
        if (xn) {
            const int64_t j = idx[p];
            if (j < 0 || j >= m) { b += __builtin_nan(""); continue; }      // not dereferenced; the sum says so
            const double u0 = xn[p * 3], u1 = xn[p * 3 + 1], u2 = xn[p * 3 + 2];
            const double v0 = yn[j * 3], v1 = yn[j * 3 + 1], v2 = yn[j * 3 + 2];
            const double nu = sqrt(u0 * u0 + u1 * u1 + u2 * u2), nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
            const double c = (u0 * v0 + u1 * v1 + u2 * v2) / ((nu > 1e-6 ? nu : 1e-6) * (nv > 1e-6 ? nv : 1e-6));
            b += 1.0 - fabs(c);
        }
    }
    const double sums[2] = {a, b};
    dudf_ordsum_partial<kOrdSumBlock>(sums, partials);
}

__global__ __launch_bounds__(kOrdSumMaxGroups) void chamfer_final_kernel(const double* __restrict__ partials, int count, int with_normals,
                                                                         double* __restrict__ out_sums) {
    double sums[2];
    dudf_ordsum_finish(partials, count, sums);
    if (threadIdx.x == 0) {
        out_sums[0] = sums[0];
        if (with_normals) out_sums[1] = sums[1];
    }
}

// ---- area-weighted vertex normals -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void face_normals_kernel(const double* __restrict__ v, int64_t nv, const int64_t* __restrict__ f,
                                                           int64_t nf, double* __restrict__ acc) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nf; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = f[t * 3], i1 = f[t * 3 + 1], i2 = f[t * 3 + 2];
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) continue;
        const double e0 = v[i1 * 3] - v[i0 * 3], e1 = v[i1 * 3 + 1] - v[i0 * 3 + 1], e2 = v[i1 * 3 + 2] - v[i0 * 3 + 2];
        const double g0 = v[i2 * 3] - v[i0 * 3], g1 = v[i2 * 3 + 1] - v[i0 * 3 + 1], g2 = v[i2 * 3 + 2] - v[i0 * 3 + 2];
        const double c[3] = {e1 * g2 - e2 * g1, e2 * g0 - e0 * g2, e0 * g1 - e1 * g0};      // twice the area times the unit normal
        const int64_t corner[3] = {i0, i1, i2};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) atomicAdd(&acc[corner[a] * 3 + i], c[i]);
    }
}

__global__ __launch_bounds__(256) void vertex_normalize_kernel(const double* __restrict__ acc, int64_t nv, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nv; p += (int64_t)gridDim.x * blockDim.x) {
        const double a = acc[p * 3], b = acc[p * 3 + 1], c = acc[p * 3 + 2];
        const double len = sqrt(a * a + b * b + c * c);
        const bool ok = len > 0.0;                      // false for a zero sum and for NaN
        out[p * 3] = ok ? (float)(a / len) : 0.0f;
        out[p * 3 + 1] = ok ? (float)(b / len) : 0.0f;
        out[p * 3 + 2] = ok ? (float)(c / len) : 1.0f;
    }
}

}  // namespace

extern "C" {

// the three byte counts of this unit are never 0: an empty input still asks for one 256-byte granule
size_t dudf_nearest_workspace_bytes(int64_t n) { return n > 0 ? dudf_round256((size_t)n * sizeof(unsigned long long)) : 256; }

int dudf_nearest_points(const float* x, int64_t n, const float* y, int64_t m, int norm, float* out_dist, int64_t* out_idx,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (norm != 1 && norm != 2) return DUDF_E_BADMODE;
    if (n < 0) return DUDF_E_BADCFG;
    if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (n == 0) return 0;
    if (m <= 0 || !x || !y) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_nearest_workspace_bytes(n))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
    DUDF_TRY(hipMemsetAsync(keys, 0xff, (size_t)n * sizeof(unsigned long long), st));
    // split y so that the launch has about kNnTargetGroups workgroups, each split at least one LDS tile long
    const int64_t xgroups = (n + kNnRows - 1) / kNnRows;
    int64_t splits = kNnTargetGroups / xgroups;
    const int64_t max_splits = (m + kNnTile - 1) / kNnTile;
    if (splits > max_splits) splits = max_splits;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const int64_t ychunk = (m + splits - 1) / splits;
    splits = (m + ychunk - 1) / ychunk;                  // no empty split: every workgroup's first index lies in [0, m)
    const dim3 grid((unsigned)xgroups, (unsigned)splits);
    DUDF_TRY(dudf_launch(norm == 2 ? nearest_kernel<2> : nearest_kernel<1>, grid, dim3(kNnBlock), st, x, n, y, (int)m, (int)ychunk, keys));
    if (out_dist || out_idx)
        DUDF_TRY(dudf_launch(nearest_finish_kernel, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), st, keys, n, (int)m, out_dist,
                             out_idx));
    return 0;
}

size_t dudf_chamfer_terms_workspace_bytes(int64_t n) { return dudf_round256((size_t)dudf_ordsum_groups(n) * 2 * sizeof(double)); }   // >= 1 group: >= 256

int dudf_chamfer_terms(const float* dist, const int64_t* idx, int64_t n, const float* x_normals, const float* y_normals, int64_t m,
                       double* out_sums, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || !out_sums || (n > 0 && !dist)) return DUDF_E_BADCFG;
    if ((x_normals == nullptr) != (y_normals == nullptr)) return DUDF_E_BADCFG;
    if (x_normals && n > 0 && (!idx || m <= 0)) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_chamfer_terms_workspace_bytes(n))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    double* partials = reinterpret_cast<double*>(workspace);
    const int groups = n > 0 ? dudf_ordsum_groups(n) : 0;
    if (groups > 0)
        DUDF_TRY(dudf_launch(chamfer_partial_kernel, dim3(groups), dim3(kOrdSumBlock), st, dist, idx, n, x_normals, y_normals, m, partials));
    return dudf_launch(chamfer_final_kernel, dim3(1), dim3(kOrdSumMaxGroups), st, partials, groups, x_normals ? 1 : 0, out_sums);
}

size_t dudf_vertex_normals_workspace_bytes(int64_t n_vertices) {
    return n_vertices > 0 ? dudf_round256((size_t)n_vertices * 3 * sizeof(double)) : 256;
}

int dudf_vertex_normals(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, float* out_normals,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (n_vertices < 0 || n_faces < 0) return DUDF_E_BADCFG;
    if (n_vertices == 0) return 0;
    if (!vertices || !out_normals || (n_faces > 0 && !faces)) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_vertex_normals_workspace_bytes(n_vertices))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    double* acc = reinterpret_cast<double*>(workspace);
    DUDF_TRY(hipMemsetAsync(acc, 0, (size_t)n_vertices * 3 * sizeof(double), st));
    if (n_faces > 0)
        DUDF_TRY(dudf_launch(face_normals_kernel, dim3(dudf_grid_for(n_faces, 256, kGridCap)), dim3(256), st, vertices, n_vertices, faces,
                             n_faces, acc));
    return dudf_launch(vertex_normalize_kernel, dim3(dudf_grid_for(n_vertices, 256, kGridCap)), dim3(256), st, acc, n_vertices, out_normals);
}

}  // extern "C"
