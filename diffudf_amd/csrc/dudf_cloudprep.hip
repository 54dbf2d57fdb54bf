// Raw scans on the device: normals estimated from the k-NN graph and the statistical outlier test — what open3d's
// `estimate_normals(KDTreeSearchParamKNN(k))` and `remove_statistical_outlier(nb_neighbors, std_ratio)` do for a cloud that comes
// without normals (reference preprocess.py -pc assumes a cloud that has them).  Kernels and their C entry points (include/dudf_hip.h);
// the rules are DESIGN.md §3.8, tests/cloudprep_oracle.py restates them in numpy.  Built with -ffp-contract=off (csrc/Makefile): the
// mean, the covariance and the threshold are the oracle's expressions, one rounding per operation.
//
// Estimation.  One thread per point.  The cloud is first packed to float4 in the workspace, so a neighbour is one 16-byte load; the
// thread walks its row of knn_idx twice (mean, then the centred outer products), keeps six fp64 sums and hands the lower triangle to
// eigh3 (dudf_eigh3.h).  No array is indexed by a run-time value: nothing leaves the registers.
//
// Outliers.  d_i = mean of sqrt(dist) over the finite slots of row i; mu and sigma of the finite d_i as ordered sums
// (dudf_ordsum.h: per-workgroup partials that one workgroup adds in index order), sigma from the centred second pass; keep = d_i <= mu + ratio * sigma;
// the kept rows are compacted in ascending order with dudf_wgscan.h (tile counts, dudf_scan_totals_kernel<1>, scatter).  No atomics.
#include "dudf_context.h"
#include "dudf_eigh3.h"
#include "dudf_ordsum.h"
#include "dudf_pairdist.h"
#include "dudf_wgscan.h"

namespace {

constexpr int kBlock = DUDF_WG;                  // threads per workgroup; the compaction's tile
static_assert(kBlock == kOrdSumBlock, "the sums' launches are sized by dudf_ordsum_groups");
constexpr int kGridCap = 4096;                   // workgroups of the row-wise launches; the kernels stride over the rest
constexpr int kMaxK = 16;
constexpr double kDblMax = 1.7976931348623157e+308;

// ---- normals -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cloud_pack_kernel(const float* __restrict__ pts, int64_t n, float4* __restrict__ p4) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock)
        p4[r] = make_float4(pts[r * 3], pts[r * 3 + 1], pts[r * 3 + 2], 0.0f);
}

// the other end of slot s of row i, or -1 for a slot that is no neighbour (never dereferenced)
__device__ __forceinline__ int64_t slot_neighbour(const int64_t* __restrict__ row, int s, int64_t i, int64_t n) {
    const int64_t j = row[s];
    return (j < 0 || j >= n || j == i) ? -1 : j;
}

__global__ __launch_bounds__(kBlock) void estimate_normals_kernel(const float4* __restrict__ p4, const int64_t* __restrict__ idx, int64_t n,
                                                                  int K, int include_self, float* __restrict__ out_normals,
                                                                  double* __restrict__ out_eig, int* __restrict__ out_count) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t* row = idx + i * K;
        const float4 self = p4[i];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int c = 0;
        bool fin = true;
        if (include_self) {
            fin = finite3(self.x, self.y, self.z);
            sx += (double)self.x; sy += (double)self.y; sz += (double)self.z;
            c = 1;
        }
        for (int s = 0; s < K; ++s) {
            const int64_t j = slot_neighbour(row, s, i, n);
            if (j < 0) continue;
            const float4 q = p4[j];
            fin = fin && finite3(q.x, q.y, q.z);
            sx += (double)q.x; sy += (double)q.y; sz += (double)q.z;
            ++c;
        }
        double lam[3] = {0.0, 0.0, 0.0}, nx = 0.0, ny = 0.0, nz = 1.0;      // open3d's fallback
        if (fin && c >= 3) {
            const double dc = (double)c, mx = sx / dc, my = sy / dc, mz = sz / dc;
            double a00 = 0.0, a10 = 0.0, a11 = 0.0, a20 = 0.0, a21 = 0.0, a22 = 0.0;
            if (include_self) {
                const double dx = (double)self.x - mx, dy = (double)self.y - my, dz = (double)self.z - mz;
                a00 += dx * dx; a10 += dy * dx; a11 += dy * dy; a20 += dz * dx; a21 += dz * dy; a22 += dz * dz;
            }
            for (int s = 0; s < K; ++s) {
                const int64_t j = slot_neighbour(row, s, i, n);
                if (j < 0) continue;
                const float4 q = p4[j];
                const double dx = (double)q.x - mx, dy = (double)q.y - my, dz = (double)q.z - mz;
                a00 += dx * dx; a10 += dy * dx; a11 += dy * dy; a20 += dz * dx; a21 += dz * dy; a22 += dz * dz;
            }
            a00 /= dc; a10 /= dc; a11 /= dc; a20 /= dc; a21 /= dc; a22 /= dc;
            if (a00 != 0.0 || a10 != 0.0 || a11 != 0.0 || a20 != 0.0 || a21 != 0.0 || a22 != 0.0) {
                const double H[3][3] = {{a00, 0.0, 0.0}, {a10, a11, 0.0}, {a20, a21, a22}};       // eigh3 reads the lower triangle
                double V[3][3];
                eigh3(H, lam, V);
                const double len = sqrt((V[0][0] * V[0][0] + V[1][0] * V[1][0]) + V[2][0] * V[2][0]);
                nx = V[0][0] / len; ny = V[1][0] / len; nz = V[2][0] / len;
            }
        }
        out_normals[i * 3] = (float)nx; out_normals[i * 3 + 1] = (float)ny; out_normals[i * 3 + 2] = (float)nz;
        if (out_eig) { out_eig[i * 3] = lam[0]; out_eig[i * 3 + 1] = lam[1]; out_eig[i * 3 + 2] = lam[2]; }
        if (out_count) out_count[i] = c;
    }
}

// ---- outliers: the statistics ----------------------------------------------------------------------------------------------------------
// d_i of every row, and per workgroup the ordered sum (dudf_ordsum.h) and the number of the finite ones: a function of (n, inputs) only.
__global__ __launch_bounds__(kBlock) void outlier_mean_kernel(const float* __restrict__ dist, int64_t n, int K, double* __restrict__ mean_dist,
                                                              double* __restrict__ psum, unsigned long long* __restrict__ pcnt) {
    __shared__ double sd[kBlock];
    __shared__ unsigned long long sc[kBlock];
    double a = 0.0;
    unsigned long long cnt = 0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const float* row = dist + p * K;
        double s = 0.0;
        int c = 0;
        for (int k = 0; k < K; ++k) {
            const float d = row[k];
            if (fabsf(d) <= kFltMax) { s += sqrt((double)d); ++c; }      // false for +inf (a padded slot) and NaN
        }
        const double m = c > 0 ? s / (double)c : __builtin_inf();
        mean_dist[p] = m;
        if (fabs(m) <= kDblMax) { a += m; ++cnt; }
    }
    sd[threadIdx.x] = a; sc[threadIdx.x] = cnt;
    dudf_wg_tree<kBlock>(dudf_sum_of(sd), dudf_sum_of(sc));
    if (threadIdx.x == 0) { psum[blockIdx.x] = sd[0]; pcnt[blockIdx.x] = sc[0]; }
}

// stat: [0] mu, [1] sigma, [2] threshold; *total: the finite rows
__global__ __launch_bounds__(kOrdSumMaxGroups) void outlier_mu_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt,
                                                                      int groups, double* __restrict__ stat, unsigned long long* __restrict__ total) {
    double a[1];
    unsigned long long c[1];
    dudf_ordsum_finish(psum, groups, a);
    dudf_ordsum_finish(pcnt, groups, c);
    if (threadIdx.x == 0) {
        stat[0] = a[0] / (double)c[0];                                  // no finite row: NaN, and no row passes the test
        *total = c[0];
    }
}

__global__ __launch_bounds__(kBlock) void outlier_var_kernel(const double* __restrict__ mean_dist, int64_t n, const double* __restrict__ stat,
                                                             double* __restrict__ psum) {
    const double mu = stat[0];
    double a = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const double m = mean_dist[p];
        if (fabs(m) <= kDblMax) { const double d = m - mu; a += d * d; }
    }
    const double sums[1] = {a};
    dudf_ordsum_partial<kBlock>(sums, psum);
}

__global__ __launch_bounds__(kOrdSumMaxGroups) void outlier_sigma_kernel(const double* __restrict__ psum, int groups,
                                                                         const unsigned long long* __restrict__ total, double std_ratio,
                                                                         double* __restrict__ stat, double* __restrict__ out_stats) {
    double a[1];
    dudf_ordsum_finish(psum, groups, a);
    if (threadIdx.x == 0) {
        const double mu = stat[0], sigma = sqrt(a[0] / (double)*total), thr = mu + std_ratio * sigma;
        stat[1] = sigma; stat[2] = thr;
        if (out_stats) { out_stats[0] = mu; out_stats[1] = sigma; out_stats[2] = thr; }
    }
}

// ---- outliers: the kept rows in ascending order -------------------------------------------------------------------------------------------
// tiles of kBlock rows: kept rows per tile (dudf_wg_rank's total), dudf_scan_totals_kernel<1>, then row -> tile offset + kept rows before it
__global__ __launch_bounds__(kBlock) void outlier_count_kernel(const double* __restrict__ mean_dist, int64_t n, int64_t ntiles,
                                                               const double* __restrict__ stat, uint32_t* __restrict__ blk) {
    __shared__ unsigned wave_tot[kBlock / 64];
    const double thr = stat[2];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t row = t * kBlock + threadIdx.x;
        unsigned total;
        dudf_wg_rank(row < n && mean_dist[row] <= thr, wave_tot, &total);
        if (threadIdx.x == 0) blk[t] = total;
    }
}

__global__ __launch_bounds__(kBlock) void outlier_scatter_kernel(const double* __restrict__ mean_dist, int64_t n, int64_t ntiles,
                                                                 const double* __restrict__ stat, const int64_t* __restrict__ off,
                                                                 unsigned char* __restrict__ out_keep, int64_t* __restrict__ out_kept_idx) {
    __shared__ unsigned wave_tot[kBlock / 64];
    const double thr = stat[2];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t row = t * kBlock + threadIdx.x;
        const bool keep = row < n && mean_dist[row] <= thr;
        unsigned total;
        const unsigned before = dudf_wg_rank(keep, wave_tot, &total);
        if (row < n) out_keep[row] = keep ? 1 : 0;
        if (keep && out_kept_idx) out_kept_idx[off[t] + before] = row;   // off[t] + before < the kept rows in all <= n
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
inline bool cloud_sizes_supported(int64_t n, int K) { return n < ((int64_t)1 << 31) && K >= 1 && K <= kMaxK; }

struct NormalsLayout { float4* p4; size_t bytes; };            // [n] the cloud, one 16-byte row per point
inline NormalsLayout carve_normals(void* ws, int64_t n) {
    NormalsLayout l;
    DudfByteCarver cv = dudf_carve(ws);
    l.p4 = cv.take<float4>(n);
    l.bytes = cv.o;
    return l;
}

struct OutlierLayout {
    double* psum; unsigned long long* pcnt;                    // [kOrdSumMaxGroups] the partials of a pass
    double* stat;                                              // [4] mu, sigma, threshold
    unsigned long long* finite;                                // [1] rows with a finite d
    int64_t* kept;                                             // [1] the kept rows, when the caller does not ask for them
    int64_t ntiles; uint32_t* blk; int64_t* off;               // [ntiles] kept rows per tile and their exclusive scan
    size_t bytes;
};
inline OutlierLayout carve_outliers(void* ws, int64_t n) {
    OutlierLayout l;
    l.ntiles = (n + kBlock - 1) / kBlock;
    DudfByteCarver cv = dudf_carve(ws);
    l.psum = cv.take<double>(kOrdSumMaxGroups); l.pcnt = cv.take<unsigned long long>(kOrdSumMaxGroups);
    l.stat = cv.take<double>(4); l.finite = cv.take<unsigned long long>(1); l.kept = cv.take<int64_t>(1);
    l.blk = cv.take<uint32_t>(l.ntiles); l.off = cv.take<int64_t>(l.ntiles);
    l.bytes = cv.o;
    return l;
}

}  // namespace

extern "C" {

size_t dudf_estimate_normals_workspace_bytes(int64_t n, int K) {
    if (n < 0 || !cloud_sizes_supported(n, K)) return 0;
    return carve_normals(nullptr, n).bytes;
}

int dudf_estimate_normals(const float* points, const int64_t* knn_idx, int64_t n, int K, int include_self, float* out_normals,
                          double* out_eigenvalues, int* out_count, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0) return DUDF_E_BADCFG;
    if (!cloud_sizes_supported(n, K)) return DUDF_E_UNSUPPORTED;
    if (n == 0) return 0;
    if (!points || !knn_idx || !out_normals) return DUDF_E_BADCFG;
    const NormalsLayout l = carve_normals(workspace, n);
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, l.bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const dim3 rows(dudf_grid_for(n, kBlock, kGridCap)), blk(kBlock);
    DUDF_TRY(dudf_launch(cloud_pack_kernel, rows, blk, st, points, n, l.p4));
    return dudf_launch(estimate_normals_kernel, rows, blk, st, l.p4, knn_idx, n, K, include_self ? 1 : 0, out_normals, out_eigenvalues,
                       out_count);
}

size_t dudf_cloud_outliers_workspace_bytes(int64_t n, int K) {
    if (n < 0 || !cloud_sizes_supported(n, K)) return 0;
    return carve_outliers(nullptr, n).bytes;
}

int dudf_cloud_outliers(const float* knn_dist, int64_t n, int K, double std_ratio, double* out_mean_dist, unsigned char* out_keep,
                        double* out_stats, int64_t* out_kept_idx, int64_t* out_counts, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (n < 0) return DUDF_E_BADCFG;
    if (!cloud_sizes_supported(n, K)) return DUDF_E_UNSUPPORTED;
    if (n == 0) return 0;
    if (!knn_dist || !out_mean_dist || !out_keep) return DUDF_E_BADCFG;
    const OutlierLayout l = carve_outliers(workspace, n);
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, l.bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const int groups = dudf_ordsum_groups(n);
    const dim3 tiles(dudf_grid_for(n, kBlock, kGridCap)), blk(kBlock);
    DUDF_TRY(dudf_launch(outlier_mean_kernel, dim3(groups), blk, st, knn_dist, n, K, out_mean_dist, l.psum, l.pcnt));
    DUDF_TRY(dudf_launch(outlier_mu_kernel, dim3(1), dim3(kOrdSumMaxGroups), st, l.psum, l.pcnt, groups, l.stat, l.finite));
    DUDF_TRY(dudf_launch(outlier_var_kernel, dim3(groups), blk, st, out_mean_dist, n, l.stat, l.psum));
    DUDF_TRY(dudf_launch(outlier_sigma_kernel, dim3(1), dim3(kOrdSumMaxGroups), st, l.psum, groups, l.finite, std_ratio, l.stat, out_stats));
    DUDF_TRY(dudf_launch(outlier_count_kernel, tiles, blk, st, out_mean_dist, n, l.ntiles, l.stat, l.blk));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, l.blk, l.off, l.ntiles, out_counts ? out_counts : l.kept));
    return dudf_launch(outlier_scatter_kernel, tiles, blk, st, out_mean_dist, n, l.ntiles, l.stat, l.off, out_keep, out_kept_idx);
}

}  // extern "C"
