// K nearest neighbours and consistent normal orientation on the device — what pytorch3d's `knn_points(x, y, K)` and open3d's
// `orient_normals_consistent_tangent_plane(k)` do for reference generate_pc.py:40.  Kernels and their C entry points
// (include/dudf_hip.h); the rules are DESIGN.md §3.7.
//
// K-nearest search.  A row's result is its K smallest keys (distance bits << 32 | index of the y row) in ascending order: distances
// are non-negative, so unsigned order of the keys is (distance, index) order.  The distance is pair_distance<2> of dudf_pairdist.h,
// the expression dudf_nearest_points uses, so K = 1 repeats that call and both modes below agree bit for bit.  A lane keeps its list
// as a register array updated by an unrolled min/max network (new[s] = min(old[s], max(old[s - 1], c))): no dynamic index anywhere.
//   - brute: the tiled scan of nearest_kernel (y tile in LDS, broadcast reads, several x rows per lane); y is split across
//     blockIdx.y, every split writes its sorted list and a finishing kernel merges them in split order — no atomics;
//   - grid: a uniform cell list over the bounding box of y's finite rows (min/max by integer atomics on order-preserving codes,
//     cell of every point, histogram, scan with dudf_wgscan.h, scatter of float4 (x, y, z, index bits)).  A query walks its cell
//     block in growing cubic shells and stops when its K-th distance is strictly below a lower bound of the computed distance to
//     anything outside the block, or when the block covers the grid.  The bound comes from per-axis edge tables built from the
//     cell function itself (monotone in the coordinate), so it holds for the cells the points were actually put in, rounding
//     included.  Queries are counting-sorted by cell: a wave's lanes walk the same rows of cells.
//
// Orientation.  Borůvka over the k-NN graph with a union-find whose word per vertex is (parent << 1) | parity to parent: a round takes
// the minimum key of every component by 64-bit atomicMin, hooks along it (a mutual pair keeps the smaller representative), and
// flattens (parent, parity) by pointer doubling.  Every loop has a trip count known at launch.
#include "dudf_context.h"
#include "dudf_pairdist.h"
#include "dudf_wgscan.h"
#include <utility>

namespace {

constexpr int kBlock = 256;
constexpr int kGridCap = 4096;                   // workgroups of the row-wise launches; the kernels stride over the rest
constexpr int kMaxK = 16;
constexpr unsigned kInfBits = 0x7f800000u, kNanBits = 0x7fc00000u;
constexpr unsigned long long kPadKey = ((unsigned long long)kInfBits << 32) | 0xffffffffull;     // +inf, no index

// ---- the K-list --------------------------------------------------------------------------------------------------------------------
// KC >= K slots in ascending order.  The first KC - K hold the key 0 and stay there (an insertion puts its key behind equal ones),
// so the list proper is slots [KC - K, KC) and its K-th entry is key[KC - 1]: every index is a constant.  (Picking key[K - 1] out of
// a K-entry list with selects does not stay in registers: the compiler turns a select of loads into a load at a selected address.)
template <int KC>
__device__ __forceinline__ void klist_init(unsigned long long (&key)[KC], int K) {
#pragma unroll
    for (int s = 0; s < KC; ++s) key[s] = (s < KC - K) ? 0ull : kPadKey;
}
// sorted insertion of c: new[s] = min(old[s], max(old[s - 1], c)), descending s so that old[s - 1] is still old
template <int KC>
__device__ __forceinline__ void klist_insert(unsigned long long (&key)[KC], unsigned long long c) {
#pragma unroll
    for (int s = KC - 1; s > 0; --s) {
        const unsigned long long up = key[s - 1] > c ? key[s - 1] : c;
        key[s] = key[s] < up ? key[s] : up;
    }
    key[0] = key[0] < c ? key[0] : c;
}
template <int KC>
__device__ __forceinline__ unsigned long long klist_kth(const unsigned long long (&key)[KC], int) { return key[KC - 1]; }
// candidates are looked at only while their distance is <= this: the K-th distance, and never +inf or NaN
__device__ __forceinline__ float klist_threshold(unsigned long long kth) { return fminf(__uint_as_float((unsigned)(kth >> 32)), kFltMax); }

// the list proper to the outputs of `row`; expanded by the front end (a loop with `s >= KC - K` inside is re-rolled to a dynamic trip
// count, and the list leaves the registers)
template <int KC, int... I>
__device__ __forceinline__ void klist_write_seq(const unsigned long long (&key)[KC], int K, int64_t row, int m, bool row_finite,
                                                float* __restrict__ out_dist, int64_t* __restrict__ out_idx, std::integer_sequence<int, I...>) {
    const int64_t base = row * K - (KC - K);
    if (out_dist)
        ((I >= KC - K ? (void)(out_dist[base + I] = row_finite ? __uint_as_float((unsigned)(key[I] >> 32)) : __uint_as_float(kNanBits)) : (void)0), ...);
    if (out_idx)
        ((I >= KC - K ? (void)(out_idx[base + I] = (row_finite && (unsigned)key[I] < (unsigned)m) ? (int64_t)(unsigned)key[I] : -1) : (void)0), ...);
}
template <int KC>
__device__ __forceinline__ void klist_write(const unsigned long long (&key)[KC], int K, int64_t row, int m, bool row_finite,
                                            float* __restrict__ out_dist, int64_t* __restrict__ out_idx) {
    klist_write_seq(key, K, row, m, row_finite, out_dist, out_idx, std::make_integer_sequence<int, KC>{});
}
// dst[0 .. K) = the list proper
template <int KC, int... I>
__device__ __forceinline__ void klist_store_seq(const unsigned long long (&key)[KC], int K, unsigned long long* __restrict__ dst,
                                                std::integer_sequence<int, I...>) {
    ((I >= KC - K ? (void)(dst[I - (KC - K)] = key[I]) : (void)0), ...);
}

// ---- brute mode --------------------------------------------------------------------------------------------------------------------
constexpr int kBrTile = 1024;                    // rows of y per LDS tile (16 KiB)
constexpr int kBrTargetGroups = 4096;
constexpr int kBrMaxSplits = 8;                  // the split lists live in the workspace: n * K * splits keys

// grid (ceil(n / (kBlock * PPL)), splits); workgroup (bx, by) scans y rows [by * ychunk, min(m, (by + 1) * ychunk)) — never empty —
// and writes the sorted K-list of its rows into part[(by * n + row) * K ..].  Rows past n repeat row n - 1 and are not written.
template <int KC, int PPL>
__global__ __launch_bounds__(kBlock) void knn_brute_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ y, int m,
                                                           int ychunk, int K, int exclude_self, unsigned long long* __restrict__ part) {
    __shared__ float4 tile[kBrTile];
    const int64_t row0 = (int64_t)blockIdx.x * (kBlock * PPL) + threadIdx.x;
    const int y0 = blockIdx.y * ychunk;
    const int y1 = (m - y0 < ychunk) ? m : y0 + ychunk;
    float ax[PPL], ay[PPL], az[PPL], thr[PPL];
    unsigned self[PPL];
    unsigned long long key[PPL][KC], kth[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        int64_t r = row0 + (int64_t)k * kBlock;
        if (r > n - 1) r = n - 1;
        ax[k] = x[r * 3]; ay[k] = x[r * 3 + 1]; az[k] = x[r * 3 + 2];
        self[k] = exclude_self ? (unsigned)r : 0xffffffffu;
        klist_init(key[k], K);
        kth[k] = kPadKey; thr[k] = kFltMax;
    }
    for (int t0 = y0; t0 < y1; t0 = (y1 - t0 > kBrTile) ? t0 + kBrTile : y1) {        // (no step past y1: m may be close to 2^31)
        const int cnt = (y1 - t0 < kBrTile) ? y1 - t0 : kBrTile;
        __syncthreads();                 // the previous tile has been read by every wave
        for (int j = threadIdx.x; j < cnt; j += kBlock) {
            const float* q = y + (int64_t)(t0 + j) * 3;
            tile[j] = make_float4(q[0], q[1], q[2], 0.0f);
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            const float4 q = tile[j];    // wave-uniform address: a broadcast read
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                const float d = pair_distance<2>(ax[k], ay[k], az[k], q);
                if (d <= thr[k]) {       // false for NaN and +inf
                    const unsigned long long c = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(t0 + j);
                    if (c < kth[k] && (unsigned)(t0 + j) != self[k]) {
                        klist_insert(key[k], c);
                        kth[k] = klist_kth(key[k], K);
                        thr[k] = klist_threshold(kth[k]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int64_t r = row0 + (int64_t)k * kBlock;
        if (r >= n) continue;
        unsigned long long* dst = part + ((int64_t)blockIdx.y * n + r) * K;
        klist_store_seq(key[k], K, dst, std::make_integer_sequence<int, KC>{});
    }
}

// one thread per row: the split lists in split order into one list, then the outputs
template <int KC>
__global__ __launch_bounds__(kBlock) void knn_merge_kernel(const float* __restrict__ x, int64_t n, int m, int K, int splits,
                                                           const unsigned long long* __restrict__ part, float* __restrict__ out_dist,
                                                           int64_t* __restrict__ out_idx) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        unsigned long long key[KC];
        klist_init(key, K);
        for (int sp = 0; sp < splits; ++sp) {
            const unsigned long long* src = part + ((int64_t)sp * n + r) * K;
            for (int s = 0; s < K; ++s) {
                const unsigned long long c = src[s];
                if (c < klist_kth(key, K)) klist_insert(key, c);
            }
        }
        klist_write(key, K, r, m, finite3(x[r * 3], x[r * 3 + 1], x[r * 3 + 2]), out_dist, out_idx);
    }
}

// ---- grid mode: the cell list ------------------------------------------------------------------------------------------------------
constexpr int kMaxG = 256;                       // cells per axis at most: 2^24 cells
constexpr int kScanItems = 4;                    // cells per thread of the scan: 1024 per workgroup
constexpr int kEdgeSteps = 8;

struct GridParams {                              // the head of the workspace, written on the device
    unsigned lo_code[3], hi_code[3];             // order-preserving codes of the bounding box of the finite rows
    unsigned n_finite;
    int G;                                       // cells per axis actually used: the host's G, or 1 for a degenerate box
    float lo[3], inv_h;
};

// the cell of a coordinate along one axis: monotone non-decreasing in p (each step is), NaN and anything out of range clamped
__device__ __forceinline__ int axis_cell(float p, float lo, float inv_h, int G) {
    float t = (p - lo) * inv_h;
    t = fminf(fmaxf(t, 0.0f), (float)(G - 1));   // fmaxf(NaN, 0) = 0
    return (int)t;
}

__global__ void grid_init_kernel(GridParams* prm) {
    if (threadIdx.x < 3) { prm->lo_code[threadIdx.x] = 0xffffffffu; prm->hi_code[threadIdx.x] = 0u; }
    if (threadIdx.x == 3) prm->n_finite = 0u;
}

__global__ __launch_bounds__(kBlock) void grid_bbox_kernel(const float* __restrict__ y, int m, GridParams* prm) {
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, cnt = 0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < m; p += (int64_t)gridDim.x * kBlock) {
        const float a = y[p * 3], b = y[p * 3 + 1], c = y[p * 3 + 2];
        if (!finite3(a, b, c)) continue;
        const unsigned ca = float_code(a), cb = float_code(b), cc = float_code(c);
        lo[0] = min(lo[0], ca); hi[0] = max(hi[0], ca);
        lo[1] = min(lo[1], cb); hi[1] = max(hi[1], cb);
        lo[2] = min(lo[2], cc); hi[2] = max(hi[2], cc);
        ++cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o));
        }
        cnt += (unsigned)__shfl_xor((int)cnt, o);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(&prm->lo_code[a], lo[a]); atomicMax(&prm->hi_code[a], hi[a]); }
        atomicAdd(&prm->n_finite, cnt);
    }
}

// One workgroup: the box -> (lo, inv_h, G), and the edge tables.  For 1 <= i <= G - 1 along axis a
//   below[a][i]: a coordinate whose cell is < i, so every point in a cell >= i lies strictly above it;
//   above[a][i]: a coordinate whose cell is >= i, so every point in a cell < i lies strictly below it
// (the cell function is monotone).  They start at lo + i * h and step away from it; -inf / +inf if kEdgeSteps do not get there, which
// only makes a query look further.
__global__ __launch_bounds__(kBlock) void grid_params_kernel(GridParams* prm, int G_host, float* __restrict__ below, float* __restrict__ above) {
    float lo[3], ext = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = code_float(prm->lo_code[a]);
        ext = fmaxf(ext, code_float(prm->hi_code[a]) - lo[a]);
    }
    const bool ok = prm->n_finite > 0 && ext > 0.0f && ext <= kFltMax;
    const int G = ok ? G_host : 1;
    const float h = ok ? ext / (float)G : 1.0f, inv_h = ok ? (float)G / ext : 0.0f;
    const bool usable = inv_h > 0.0f && inv_h <= kFltMax;     // a box so small that G / ext overflows: one cell
    const int Ge = usable ? G : 1;
    const float inv = usable ? inv_h : 0.0f;
    if (!ok) { lo[0] = lo[1] = lo[2] = 0.0f; }
    __syncthreads();                                          // every thread has read the codes before thread 0 writes beside them
    if (threadIdx.x == 0) {
        prm->G = Ge; prm->inv_h = inv;
        prm->lo[0] = lo[0]; prm->lo[1] = lo[1]; prm->lo[2] = lo[2];
    }
    for (int t = threadIdx.x; t < 3 * (G_host + 1); t += kBlock) {
        const int a = t / (G_host + 1), i = t % (G_host + 1);
        float b = -__builtin_inff(), u = __builtin_inff();
        if (i >= 1 && i <= Ge - 1) {
            // steps of 2^-21 of the largest magnitude involved: a few floats of lo + i * h AND of (e - lo), whichever is coarser (a
            // boundary near 0 of a box that starts far from 0 does not move the difference when it moves by its own last bit)
            const float e0 = lo[a] + (float)i * h;
            const float step = fmaxf(fmaxf(fabsf(lo[a]), fabsf(lo[a] + ext)), ext) * 4.76837158203125e-07f;
            float e = e0;
            bool found = false;
            for (int s = 0; s < kEdgeSteps; ++s) {
                e = e0 - (float)s * step;
                if (axis_cell(e, lo[a], inv, Ge) < i) { found = true; break; }
            }
            if (found) b = e;
            found = false;
            for (int s = 0; s < kEdgeSteps; ++s) {
                e = e0 + (float)s * step;
                if (axis_cell(e, lo[a], inv, Ge) >= i) { found = true; break; }
            }
            if (found) u = e;
        }
        below[t] = b; above[t] = u;
    }
}

// rows -> cells, and the histogram.  A non-finite row of y gets cell -1 (it is in no cell); a non-finite query is counted in cell 0.
__global__ __launch_bounds__(kBlock) void cell_count_kernel(const float* __restrict__ p, int64_t n, const GridParams* __restrict__ prm,
                                                            int skip_nonfinite, int* __restrict__ cell, unsigned* __restrict__ count) {
    const int G = prm->G;
    const float l0 = prm->lo[0], l1 = prm->lo[1], l2 = prm->lo[2], inv = prm->inv_h;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        const float a = p[r * 3], b = p[r * 3 + 1], c = p[r * 3 + 2];
        int id = -1;
        if (finite3(a, b, c)) id = (axis_cell(c, l2, inv, G) * G + axis_cell(b, l1, inv, G)) * G + axis_cell(a, l0, inv, G);
        else if (!skip_nonfinite) id = 0;
        cell[r] = id;
        if (id >= 0) atomicAdd(&count[id], 1u);
    }
}

// exclusive scan of the cell counts, three launches: per-workgroup scan + totals, dudf_scan_totals_kernel<1>, the offsets added
__global__ __launch_bounds__(DUDF_WG) void cell_scan_local_kernel(const unsigned* count, int64_t ncells, unsigned* out,   // out may be count
                                                                 
                                                                  uint32_t* __restrict__ blk) {
    __shared__ unsigned wave_tot[DUDF_WG / 64];
    const int64_t base = ((int64_t)blockIdx.x * DUDF_WG + threadIdx.x) * kScanItems;
    unsigned v[kScanItems], sum = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) { v[i] = (base + i < ncells) ? count[base + i] : 0u; sum += v[i]; }
    unsigned total;
    unsigned run = dudf_wg_scan(sum, wave_tot, &total);
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        if (base + i < ncells) out[base + i] = run;
        run += v[i];
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(DUDF_WG) void cell_scan_add_kernel(unsigned* __restrict__ out, int64_t ncells, const int64_t* __restrict__ off,
                                                                const int64_t* __restrict__ total, int write_end) {
    const int64_t base = ((int64_t)blockIdx.x * DUDF_WG + threadIdx.x) * kScanItems;
    const unsigned add = (unsigned)off[blockIdx.x];
#pragma unroll
    for (int i = 0; i < kScanItems; ++i)
        if (base + i < ncells) out[base + i] += add;
    if (write_end && blockIdx.x == 0 && threadIdx.x == 0) out[ncells] = (unsigned)total[0];
}

__global__ __launch_bounds__(kBlock) void cell_scatter_points_kernel(const float* __restrict__ y, int m, const int* __restrict__ cell,
                                                                     unsigned* __restrict__ cursor, float4* __restrict__ pts) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < m; r += (int64_t)gridDim.x * kBlock) {
        const int id = cell[r];
        if (id < 0) continue;
        const unsigned pos = atomicAdd(&cursor[id], 1u);         // the order inside a cell is arrival order; no result depends on it
        if (pos < (unsigned)m) pts[pos] = make_float4(y[r * 3], y[r * 3 + 1], y[r * 3 + 2], __uint_as_float((unsigned)r));
    }
}

__global__ __launch_bounds__(kBlock) void cell_scatter_queries_kernel(int64_t n, const int* __restrict__ cell, unsigned* __restrict__ cursor,
                                                                      unsigned* __restrict__ order) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        const int id = cell[r];
        if (id < 0) continue;
        const unsigned pos = atomicAdd(&cursor[id], 1u);
        if (pos < (unsigned)n) order[pos] = (unsigned)r;
    }
}

// ---- grid mode: the search ---------------------------------------------------------------------------------------------------------
// the points of cells [xa, xb] of row (z, y): one contiguous run of the cell list
template <int KC>
__device__ __forceinline__ void scan_cells(const float4* __restrict__ pts, const unsigned* __restrict__ cstart, int G, int m, int z, int y,
                                           int xa, int xb, float qx, float qy, float qz, unsigned self, int K,
                                           unsigned long long (&key)[KC], unsigned long long& kth, float& thr) {
    const int64_t row = ((int64_t)z * G + y) * G;
    unsigned b = cstart[row + xa], e = cstart[row + xb + 1];
    if (e > (unsigned)m) e = (unsigned)m;                        // the scan cannot exceed m; this keeps the loop inside pts whatever it read
    for (unsigned p = b; p < e; ++p) {
        const float4 c = pts[p];                                 // one 16-byte load
        const float d = pair_distance<2>(qx, qy, qz, c);
        if (d <= thr) {
            const unsigned j = __float_as_uint(c.w);
            const unsigned long long ck = ((unsigned long long)__float_as_uint(d) << 32) | j;
            if (ck < kth && j != self) {
                klist_insert(key, ck);
                kth = klist_kth(key, K);
                thr = klist_threshold(kth);
            }
        }
    }
}

template <int KC>
__global__ __launch_bounds__(kBlock) void knn_grid_kernel(const float* __restrict__ x, int64_t n, int m, int K, int exclude_self,
                                                          const GridParams* __restrict__ prm, const float* __restrict__ below,
                                                          const float* __restrict__ above, int G_host, const float4* __restrict__ pts,
                                                          const unsigned* __restrict__ cstart, const unsigned* __restrict__ order,
                                                          float* __restrict__ out_dist, int64_t* __restrict__ out_idx) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const int64_t r = order[t];
    if (r >= n) return;
    const float q[3] = {x[r * 3], x[r * 3 + 1], x[r * 3 + 2]};
    unsigned long long key[KC], kth = kPadKey;
    klist_init(key, K);
    if (!finite3(q[0], q[1], q[2])) { klist_write(key, K, r, m, false, out_dist, out_idx); return; }
    const int G = prm->G;
    const float inv = prm->inv_h;
    int c0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c0[a] = axis_cell(q[a], prm->lo[a], inv, G);
    const unsigned self = exclude_self ? (unsigned)r : 0xffffffffu;
    float thr = kFltMax;
    for (int s = 0; s < G; ++s) {                                // at s = G - 1 the block covers the grid wherever c0 lies
        const int z0 = max(c0[2] - s, 0), z1 = min(c0[2] + s, G - 1), y0 = max(c0[1] - s, 0), y1 = min(c0[1] + s, G - 1);
        const int xl = c0[0] - s, xh = c0[0] + s;
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const bool face = (z - c0[2] == s) || (c0[2] - z == s) || (y - c0[1] == s) || (c0[1] - y == s);
                if (face) {
                    scan_cells(pts, cstart, G, m, z, y, max(xl, 0), min(xh, G - 1), q[0], q[1], q[2], self, K, key, kth, thr);
                } else {
                    if (xl >= 0) scan_cells(pts, cstart, G, m, z, y, xl, xl, q[0], q[1], q[2], self, K, key, kth, thr);
                    if (xh <= G - 1) scan_cells(pts, cstart, G, m, z, y, xh, xh, q[0], q[1], q[2], self, K, key, kth, thr);
                }
            }
        bool covered = true;
        float bound = __builtin_inff();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int u = c0[a] + s + 1, l = c0[a] - s - 1;
            if (u <= G - 1) {                                    // cells >= u are unvisited: their points lie above below[a][u]
                covered = false;
                const float d = fmaxf(below[a * (G_host + 1) + u] - q[a], 0.0f);
                bound = fminf(bound, d * d);
            }
            if (l >= 0) {                                        // cells <= l are unvisited: their points lie below above[a][l + 1]
                covered = false;
                const float d = fmaxf(q[a] - above[a * (G_host + 1) + l + 1], 0.0f);
                bound = fminf(bound, d * d);
            }
        }
        if (covered) break;
        // A pair's computed distance is >= fl(fl(|difference along one axis|)^2), which is >= this d * d by monotone rounding; one
        // float further down for good measure.  Strictly below: an unvisited point cannot even tie.
        if (bound > 0.0f && bound <= kFltMax) bound = __uint_as_float(__float_as_uint(bound) - 1u);
        if (__uint_as_float((unsigned)(kth >> 32)) < bound) break;
    }
    klist_write(key, K, r, m, true, out_dist, out_idx);
}

// ---- orientation -------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long kNoEdge = ~0ull;

__device__ __forceinline__ float normal_dot(const float* __restrict__ nrm, int64_t i, int64_t j) {
#pragma clang fp contract(off)
    return (nrm[i * 3] * nrm[j * 3] + nrm[i * 3 + 1] * nrm[j * 3 + 1]) + nrm[i * 3 + 2] * nrm[j * 3 + 2];
}
__device__ __forceinline__ unsigned edge_weight_bits(float dot) {
#pragma clang fp contract(off)
    return __float_as_uint(1.0f - fabsf(dot));
}
// the other end of slot e of vertex i, or -1 for a slot that is no edge
__device__ __forceinline__ int64_t slot_target(const int64_t* __restrict__ idx, int64_t e, int64_t i, int64_t n) {
    const int64_t j = idx[e];
    return (j < 0 || j >= n || j == i) ? -1 : j;
}

__global__ __launch_bounds__(kBlock) void orient_init_kernel(const float* __restrict__ nrm, const int64_t* __restrict__ idx, int64_t n, int K,
                                                             unsigned* __restrict__ pp, unsigned* __restrict__ wbits) {
    const int64_t slots = n * K;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < slots; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / K, j = slot_target(idx, e, i, n);
        wbits[e] = j < 0 ? 0u : edge_weight_bits(normal_dot(nrm, i, j));
        if (e < n) pp[e] = (unsigned)e << 1;                     // every vertex its own root, parity 0
    }
}

__global__ __launch_bounds__(kBlock) void orient_best_kernel(const int64_t* __restrict__ idx, int64_t n, int K, const unsigned* __restrict__ pp,
                                                             const unsigned* __restrict__ wbits, unsigned long long* __restrict__ best) {
    const int64_t slots = n * K;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < slots; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / K, j = slot_target(idx, e, i, n);
        if (j < 0) continue;
        const unsigned ri = pp[i] >> 1, rj = pp[j] >> 1;         // flattened: the parent is the representative
        if (ri == rj || ri >= n || rj >= n) continue;
        const unsigned long long key = ((unsigned long long)wbits[e] << 32) | (unsigned)e;
        atomicMin(&best[ri], key);
        atomicMin(&best[rj], key);
    }
}

// every representative with an outgoing edge hooks to the other end's representative, except the smaller one of a mutual pair;
// cur -> nxt for every vertex (the others are copied)
__global__ __launch_bounds__(kBlock) void orient_hook_kernel(const float* __restrict__ nrm, const int64_t* __restrict__ idx, int64_t n, int K,
                                                             const unsigned* __restrict__ cur, unsigned* __restrict__ nxt,
                                                             const unsigned long long* __restrict__ best, unsigned long long* __restrict__ hooks) {
    unsigned mine = 0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        unsigned word = cur[v];
        const unsigned long long key = best[v];
        if ((word >> 1) == (unsigned)v && key != kNoEdge) {
            const int64_t e = (int64_t)(unsigned)key, i = e / K;
            const int64_t j = (i < n) ? slot_target(idx, e, i, n) : -1;
            if (j >= 0) {
                const unsigned wi = cur[i], wj = cur[j];
                const unsigned ri = wi >> 1, rj = wj >> 1;
                const unsigned other = (ri == (unsigned)v) ? rj : ri;
                if (other < n && other != (unsigned)v && !(best[other] == key && (unsigned)v < other)) {
                    const unsigned sign = normal_dot(nrm, i, j) < 0.0f ? 1u : 0u;
                    word = (other << 1) | ((wi ^ wj ^ sign) & 1u);
                    ++mine;
                }
            }
        }
        nxt[v] = word;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += (unsigned)__shfl_xor((int)mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(hooks, (unsigned long long)mine);
}

// one pointer-doubling step cur -> nxt of (parent, parity); flags[step] says whether anything moved, and a step whose predecessor moved
// nothing returns at once (both buffers are then equal)
__global__ __launch_bounds__(kBlock) void orient_jump_kernel(int64_t n, const unsigned* __restrict__ cur, unsigned* __restrict__ nxt,
                                                             unsigned* __restrict__ flags, int step) {
    if (step > 0 && flags[step - 1] == 0u) return;
    bool moved = false;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const unsigned a = cur[v], p = a >> 1;
        unsigned w = a;
        if (p < n) {
            const unsigned b = cur[p];
            w = (b & ~1u) | ((a ^ b) & 1u);
        }
        nxt[v] = w;
        moved |= (w != a);
    }
    if (__any(moved) && (threadIdx.x & 63) == 0) atomicOr(&flags[step], 1u);
}

// per component: the seed key (largest z, then smallest index) and the smallest vertex index
__global__ __launch_bounds__(kBlock) void orient_seed_kernel(const float* __restrict__ pts, int64_t n, const unsigned* __restrict__ pp,
                                                             unsigned long long* __restrict__ seed, unsigned* __restrict__ minidx) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const unsigned r = pp[v] >> 1;
        if (r >= n) continue;
        const float z = pts[v * 3 + 2] + 0.0f;                   // -0 -> +0: equal z, equal code
        atomicMax(&seed[r], ((unsigned long long)float_code(z) << 32) | (0xffffffffu - (unsigned)v));
        atomicMin(&minidx[r], (unsigned)v);
    }
}

// per representative: the flip of the whole component = the seed's parity ^ (its n_z < 0); representatives are counted
__global__ __launch_bounds__(kBlock) void orient_root_kernel(const float* __restrict__ nrm, int64_t n, const unsigned* __restrict__ pp,
                                                             const unsigned long long* __restrict__ seed, unsigned char* __restrict__ rootflip,
                                                             unsigned long long* __restrict__ components) {
    unsigned mine = 0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        if ((pp[v] >> 1) != (unsigned)v) continue;
        ++mine;
        const unsigned s = 0xffffffffu - (unsigned)seed[v];
        unsigned f = 0;
        if (s < n) f = (pp[s] & 1u) ^ (nrm[(int64_t)s * 3 + 2] < 0.0f ? 1u : 0u);
        rootflip[v] = (unsigned char)f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += (unsigned)__shfl_xor((int)mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(components, (unsigned long long)mine);
}

__global__ __launch_bounds__(kBlock) void orient_write_kernel(const float* nrm, int64_t n, const unsigned* __restrict__ pp,
                                                              const unsigned char* __restrict__ rootflip, const unsigned* __restrict__ minidx,
                                                              const unsigned long long* __restrict__ counters, float* out_normals,
                                                              unsigned char* __restrict__ out_flip, int64_t* __restrict__ out_component,
                                                              int64_t* __restrict__ out_counts) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const unsigned w = pp[v], r = w >> 1;
        const unsigned f = (r < n) ? ((w & 1u) ^ rootflip[r]) : 0u;
        if (out_flip) out_flip[v] = (unsigned char)f;
        if (out_component) out_component[v] = (r < n) ? (int64_t)minidx[r] : v;
        if (out_normals) {                                       // may alias nrm: a thread reads its own row before it writes it
            const float a = nrm[v * 3], b = nrm[v * 3 + 1], c = nrm[v * 3 + 2];
            out_normals[v * 3] = f ? -a : a; out_normals[v * 3 + 1] = f ? -b : b; out_normals[v * 3 + 2] = f ? -c : c;
        }
    }
    if (out_counts && blockIdx.x == 0 && threadIdx.x == 0) {
        out_counts[0] = (int64_t)counters[1];                    // components
        out_counts[1] = (int64_t)counters[0];                    // forest edges
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
inline int knn_cap(int K) { return K == 1 ? 1 : K <= 4 ? 4 : K <= 8 ? 8 : K <= 10 ? 10 : 16; }
inline int knn_ppl(int K) { return K <= 4 ? 4 : 2; }

struct BruteSplit { int64_t xgroups, splits, ychunk; };
inline BruteSplit brute_split(int64_t n, int64_t m, int K) {
    BruteSplit b;
    const int64_t rows = (int64_t)kBlock * knn_ppl(K);
    b.xgroups = (n + rows - 1) / rows;
    b.splits = kBrTargetGroups / (b.xgroups > 0 ? b.xgroups : 1);
    const int64_t max_splits = (m + kBrTile - 1) / kBrTile;
    if (b.splits > max_splits) b.splits = max_splits;
    if (b.splits > kBrMaxSplits) b.splits = kBrMaxSplits;
    if (b.splits < 1) b.splits = 1;
    b.ychunk = (m + b.splits - 1) / b.splits;
    if (b.ychunk < 1) b.ychunk = 1;
    b.splits = (m + b.ychunk - 1) / b.ychunk;                  // no empty split
    if (b.splits < 1) b.splits = 1;
    return b;
}

// cells per axis from m alone.  The points lie on a surface, so about 5 G^2 of the G^3 cells hold any; G = sqrt(m / 16) leaves ~3
// points in an occupied cell and makes a cell edge ~1.3 times the distance to the 10th neighbour: most queries stop after the
// 27 cells of the first shell.  
inline int grid_cells_per_axis(int64_t m) {
    int g = (int)sqrt((double)(m > 0 ? m : 1) / 16.0);
    return g < 1 ? 1 : g > kMaxG ? kMaxG : g;
}

// The cell grid's arrays.  Those that depend on n come last, so the layout of (0, m) is a prefix of the layout of (n, m): the grid
// dudf_knn_grid_build leaves in a workspace sized for (0, m) is the one dudf_knn_points(n, m) builds in front of its query arrays.
struct GridLayout {
    int G; int64_t ncells, nblocks;
    GridParams* prm; float *below, *above;                     // [3][G + 1] each
    int64_t* total; uint32_t* blk; int64_t* off;               // the scan's [nblocks] block sums and their offsets
    int* pcell; float4* pts;                                   // [m]
    unsigned *cstart, *tmp;                                    // [ncells + 1], [ncells]
    int* qcell; unsigned* qorder;                              // [n]
    size_t bytes;
};
inline GridLayout carve_grid(void* ws, int64_t n, int64_t m) {
    GridLayout g;
    g.G = grid_cells_per_axis(m);
    g.ncells = (int64_t)g.G * g.G * g.G;
    g.nblocks = (g.ncells + DUDF_WG * kScanItems - 1) / (DUDF_WG * kScanItems);
    DudfByteCarver cv = dudf_carve(ws);
    g.prm = cv.take<GridParams>(1); g.below = cv.take<float>(3 * (g.G + 1)); g.above = cv.take<float>(3 * (g.G + 1));
    g.total = cv.take<int64_t>(1); g.blk = cv.take<uint32_t>(g.nblocks); g.off = cv.take<int64_t>(g.nblocks);
    g.pcell = cv.take<int>(m); g.pts = cv.take<float4>(m);
    g.cstart = cv.take<unsigned>(g.ncells + 1); g.tmp = cv.take<unsigned>(g.ncells);
    g.qcell = cv.take<int>(n); g.qorder = cv.take<unsigned>(n);
    g.bytes = cv.o;
    return g;
}

// counts in `tmp` -> exclusive starts in `out` (may be tmp itself)
int scan_cells_host(const GridLayout& g, unsigned* out, int write_end, hipStream_t st) {
    DUDF_TRY(dudf_launch(cell_scan_local_kernel, dim3((unsigned)g.nblocks), dim3(DUDF_WG), st, g.tmp, g.ncells, out, g.blk));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, g.blk, g.off, g.nblocks, g.total));
    DUDF_TRY(dudf_launch(cell_scan_add_kernel, dim3((unsigned)g.nblocks), dim3(DUDF_WG), st, out, g.ncells, g.off, g.total, write_end));
    return 0;
}

int grid_build(const GridLayout& g, const float* y, int64_t m, hipStream_t st) {
    const dim3 rows(dudf_grid_for(m, kBlock, kGridCap));
    DUDF_TRY(dudf_launch(grid_init_kernel, dim3(1), dim3(64), st, g.prm));
    DUDF_TRY(dudf_launch(grid_bbox_kernel, rows, dim3(kBlock), st, y, (int)m, g.prm));
    DUDF_TRY(dudf_launch(grid_params_kernel, dim3(1), dim3(kBlock), st, g.prm, g.G, g.below, g.above));
    DUDF_TRY(hipMemsetAsync(g.tmp, 0, (size_t)g.ncells * sizeof(unsigned), st));
    DUDF_TRY(dudf_launch(cell_count_kernel, rows, dim3(kBlock), st, y, m, g.prm, 1, g.pcell, g.tmp));
    if (int rc = scan_cells_host(g, g.cstart, 1, st)) return rc;
    DUDF_TRY(hipMemcpyAsync(g.tmp, g.cstart, (size_t)g.ncells * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    DUDF_TRY(dudf_launch(cell_scatter_points_kernel, rows, dim3(kBlock), st, y, (int)m, g.pcell, g.tmp, g.pts));
    return 0;
}

template <int KC>
int knn_grid_run(const GridLayout& g, const float* x, int64_t n, int64_t m, int K, int exclude_self, float* out_dist, int64_t* out_idx,
                 hipStream_t st) {
    const dim3 rows(dudf_grid_for(n, kBlock, kGridCap));
    // the queries in cell order: a wave's lanes then walk the same rows of cells and share their cache lines
    DUDF_TRY(hipMemsetAsync(g.tmp, 0, (size_t)g.ncells * sizeof(unsigned), st));
    DUDF_TRY(dudf_launch(cell_count_kernel, rows, dim3(kBlock), st, x, n, g.prm, 0, g.qcell, g.tmp));
    if (int rc = scan_cells_host(g, g.tmp, 0, st)) return rc;
    DUDF_TRY(dudf_launch(cell_scatter_queries_kernel, rows, dim3(kBlock), st, n, g.qcell, g.tmp, g.qorder));
    DUDF_TRY(dudf_launch(knn_grid_kernel<KC>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), st, x, n, (int)m, K, exclude_self,
                         g.prm, g.below, g.above, g.G, g.pts, g.cstart, g.qorder, out_dist, out_idx));
    return 0;
}

// the brute mode's one array: [splits][n][K] partial lists
struct BruteLayout { BruteSplit b; unsigned long long* part; size_t bytes; };
inline BruteLayout carve_brute(void* ws, int64_t n, int64_t m, int K) {
    BruteLayout l;
    l.b = brute_split(n > 0 ? n : 1, m > 0 ? m : 1, K);
    DudfByteCarver cv = dudf_carve(ws);
    l.part = cv.take<unsigned long long>((n > 0 ? n : 1) * K * l.b.splits);
    l.bytes = cv.o;
    return l;
}

template <int KC, int PPL>
int knn_brute_run(const BruteLayout& l, const float* x, int64_t n, const float* y, int64_t m, int K, int exclude_self, float* out_dist,
                  int64_t* out_idx, hipStream_t st) {
    const BruteSplit& b = l.b;
    DUDF_TRY(dudf_launch(knn_brute_kernel<KC, PPL>, dim3((unsigned)b.xgroups, (unsigned)b.splits), dim3(kBlock), st, x, n, y, (int)m,
                         (int)b.ychunk, K, exclude_self, l.part));
    if (out_dist || out_idx) {
        DUDF_TRY(dudf_launch(knn_merge_kernel<KC>, dim3(dudf_grid_for(n, kBlock, kGridCap)), dim3(kBlock), st, x, n, (int)m, K,
                             (int)b.splits, l.part, out_dist, out_idx));
    }
    return 0;
}

inline bool knn_sizes_supported(int64_t n, int64_t m, int K) {
    return n < ((int64_t)1 << 31) && m < ((int64_t)1 << 31) && K >= 1 && K <= kMaxK;
}

inline int ceil_log2(int64_t n) {
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

struct OrientLayout {
    unsigned long long* cnt;                                   // [4] hooks in all, components, hooks of this round
    unsigned* flags;                                           // [64]
    unsigned* pp[2];                                           // [n] each: the union-find words, ping-pong
    unsigned long long* best;                                  // [n] the best edge of a round, later the seed key
    unsigned* minidx; unsigned char* rootflip;                 // [n]
    unsigned* wbits;                                           // [n][K]
    size_t bytes;
};
inline OrientLayout carve_orient(void* ws, int64_t n, int K) {
    OrientLayout l;
    DudfByteCarver cv = dudf_carve(ws);
    l.cnt = cv.take<unsigned long long>(4); l.flags = cv.take<unsigned>(64);
    l.pp[0] = cv.take<unsigned>(n); l.pp[1] = cv.take<unsigned>(n);
    l.best = cv.take<unsigned long long>(n); l.minidx = cv.take<unsigned>(n); l.rootflip = cv.take<unsigned char>(n);
    l.wbits = cv.take<unsigned>(n * K);
    l.bytes = cv.o;
    return l;
}

}  // namespace

extern "C" {

size_t dudf_knn_workspace_bytes(int64_t n, int64_t m, int K, int mode) {
    if (n < 0 || m < 0 || (mode != 0 && mode != 1) || !knn_sizes_supported(n, m, K)) return 0;
    return mode == 1 ? carve_brute(nullptr, n, m, K).bytes : carve_grid(nullptr, n, m).bytes;
}

int dudf_knn_grid_build(const float* y, int64_t m, void* workspace, size_t workspace_bytes, void* stream) {
    if (m >= ((int64_t)1 << 31)) return DUDF_E_UNSUPPORTED;
    if (m <= 0 || !y) return DUDF_E_BADCFG;
    const GridLayout g = carve_grid(workspace, 0, m);
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, g.bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    return grid_build(g, y, m, st);
}

int dudf_knn_points(const float* x, int64_t n, const float* y, int64_t m, int K, int exclude_self, int mode, float* out_dist,
                    int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (mode != 0 && mode != 1) return DUDF_E_BADMODE;
    if (n < 0) return DUDF_E_BADCFG;
    if (!knn_sizes_supported(n, m, K)) return DUDF_E_UNSUPPORTED;
    if (n == 0) return 0;
    if (m <= 0 || !x || !y) return DUDF_E_BADCFG;
    const BruteLayout l = carve_brute(workspace, n, m, K);
    const GridLayout g = carve_grid(workspace, n, m);
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, mode == 1 ? l.bytes : g.bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    exclude_self = exclude_self ? 1 : 0;
    if (mode == 1) {
        switch (knn_cap(K)) {
            case 1: return knn_brute_run<1, 4>(l, x, n, y, m, K, exclude_self, out_dist, out_idx, st);
            case 4: return knn_brute_run<4, 4>(l, x, n, y, m, K, exclude_self, out_dist, out_idx, st);
            case 8: return knn_brute_run<8, 2>(l, x, n, y, m, K, exclude_self, out_dist, out_idx, st);
            case 10: return knn_brute_run<10, 2>(l, x, n, y, m, K, exclude_self, out_dist, out_idx, st);
            default: return knn_brute_run<16, 2>(l, x, n, y, m, K, exclude_self, out_dist, out_idx, st);
        }
    }
    if (int rc = grid_build(g, y, m, st)) return rc;
    if (!out_dist && !out_idx) return 0;
    switch (knn_cap(K)) {
        case 1: return knn_grid_run<1>(g, x, n, m, K, exclude_self, out_dist, out_idx, st);
        case 4: return knn_grid_run<4>(g, x, n, m, K, exclude_self, out_dist, out_idx, st);
        case 8: return knn_grid_run<8>(g, x, n, m, K, exclude_self, out_dist, out_idx, st);
        case 10: return knn_grid_run<10>(g, x, n, m, K, exclude_self, out_dist, out_idx, st);
        default: return knn_grid_run<16>(g, x, n, m, K, exclude_self, out_dist, out_idx, st);
    }
}

size_t dudf_orient_workspace_bytes(int64_t n, int K) {
    if (n < 0 || n >= ((int64_t)1 << 31) || K < 1 || K > kMaxK || n * K >= ((int64_t)1 << 32)) return 0;
    return carve_orient(nullptr, n, K).bytes;
}

int dudf_orient_normals(const float* points, const float* normals, const int64_t* knn_idx, int64_t n, int K, float* out_normals,
                        unsigned char* out_flip, int64_t* out_component, int64_t* out_counts, int64_t* host_stats, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (n < 0) return DUDF_E_BADCFG;
    if (n >= ((int64_t)1 << 31) || K < 1 || K > kMaxK || n * K >= ((int64_t)1 << 32)) return DUDF_E_UNSUPPORTED;
    if (host_stats) host_stats[0] = host_stats[1] = 0;
    if (n == 0) return 0;
    if (!points || !normals || !knn_idx) return DUDF_E_BADCFG;
    const OrientLayout l = carve_orient(workspace, n, K);
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, l.bytes)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const dim3 vgrid(dudf_grid_for(n, kBlock, kGridCap)), sgrid(dudf_grid_for(n * K, kBlock, kGridCap)), blk(kBlock);
    int64_t launches = 0, rounds = 0;
    DUDF_TRY(hipMemsetAsync(l.cnt, 0, 4 * sizeof(unsigned long long), st));
    DUDF_TRY(dudf_launch(orient_init_kernel, sgrid, blk, st, normals, knn_idx, n, K, l.pp[0], l.wbits)); ++launches;
    // Borůvka: the components at least halve per round that hooks anything, and a round that hooks nothing is the last
    const int jumps = ceil_log2(n) > 0 ? ceil_log2(n) : 1, max_rounds = ceil_log2(n) + 1;
    int c = 0;                                                   // pp[c] is current and flat
    unsigned long long total_hooks = 0;
    for (int r = 0; r < max_rounds; ++r) {
        DUDF_TRY(hipMemsetAsync(l.best, 0xff, (size_t)n * sizeof(unsigned long long), st));
        DUDF_TRY(hipMemsetAsync(l.flags, 0, 64 * sizeof(unsigned), st));
        DUDF_TRY(dudf_launch(orient_best_kernel, sgrid, blk, st, knn_idx, n, K, l.pp[c], l.wbits, l.best));
        DUDF_TRY(dudf_launch(orient_hook_kernel, vgrid, blk, st, normals, knn_idx, n, K, l.pp[c], l.pp[1 - c], l.best, l.cnt));
        c = 1 - c;
        for (int s = 0; s < jumps; ++s) {
            DUDF_TRY(dudf_launch(orient_jump_kernel, vgrid, blk, st, n, l.pp[c], l.pp[1 - c], l.flags, s));
            c = 1 - c;
        }
        launches += 2 + jumps; ++rounds;
        unsigned long long hooks = 0;                            // the one read-back of the round
        DUDF_TRY(hipMemcpyAsync(&hooks, l.cnt, sizeof(hooks), hipMemcpyDeviceToHost, st));
        DUDF_TRY(hipStreamSynchronize(st));
        if (hooks == total_hooks) break;
        total_hooks = hooks;
    }
    DUDF_TRY(hipMemsetAsync(l.best, 0, (size_t)n * sizeof(unsigned long long), st));
    DUDF_TRY(hipMemsetAsync(l.minidx, 0xff, (size_t)n * sizeof(unsigned), st));
    DUDF_TRY(dudf_launch(orient_seed_kernel, vgrid, blk, st, points, n, l.pp[c], l.best, l.minidx));
    DUDF_TRY(dudf_launch(orient_root_kernel, vgrid, blk, st, normals, n, l.pp[c], l.best, l.rootflip, l.cnt + 1));
    DUDF_TRY(dudf_launch(orient_write_kernel, vgrid, blk, st, normals, n, l.pp[c], l.rootflip, l.minidx, l.cnt, out_normals, out_flip,
                         out_component, out_counts));
    launches += 3;
    if (host_stats) { host_stats[0] = rounds; host_stats[1] = launches; }
    return 0;
}

}  // extern "C"
