// A brick-sparse narrow band for CAP-UDF extraction: the dense path evaluates N^3 grid points and walks (N-1)^3
// cells although only a shell a few voxels thick emits a triangle.  Here a coarse lattice is evaluated, the bricks that can hold
// an active cell are selected, the fine grid is evaluated inside those bricks only, and the SAME per-cell code (dudf_capcell.h)
// runs on them through a slot table.
//
//   grid of N points per side, m = N - 1 cells, brick edge B in {4, 8};
//   brick (b0, b1, b2) owns the grid points [b_d B, b_d B + B) per axis; the storage lattice has nl = m / B + 1 bricks per side
//   (every grid point has one owner), the cell bricks are those with b_d < nb = ceil(m / B);
//   df  [slot][B][B][B] float, vec [slot][B][B][B][3] float, slot [nl^3] int32 (-1: not stored), slots in ascending brick order;
//   points of a partial brick beyond index m are evaluated at the clamped index and never read.
//
// Selection (dudf_sparse_select), from df on the (nb + 1)^3 coarse lattice at fine indices min(c_d B, m):
//   candidate: a cell brick whose 8 lattice corners have a minimum <= bound (compared in double) or hold a NaN;
//   stored   : a candidate, or a brick b + delta, delta in {0,1}^3, of a candidate b inside the lattice — so every corner of every
//              cell of a candidate brick is stored exactly once.
//   pass 1  flag    : one thread per brick, the candidate flags (a byte each)
//   pass 2  count   : stored / candidate flags ranked per workgroup (dudf_wg_rank), per-workgroup totals
//   pass 3  scan    : dudf_scan_totals_kernel<2> -> offsets and the two counts
//   pass 4  compact : slot table and the two ascending id lists at their final places — deterministic, no atomics.
// The caller reads the two counts once; nothing else of the extraction synchronises before the output sizes.
#include "dudf_context.h"
#include "dudf_capcell.h"

namespace {

constexpr int kGridCap = 2048;                         // workgroups per launch of the x4 makers; they stride over the rest
constexpr int64_t kMaxEntries = 2147483647;            // lattice entries and stored points are addressed in 31 bits

struct SparseDims {
    int64_t m; int shift;                                // cells per side; log2 of the brick edge
    int64_t nb, nl, ncoarse;                             // cell bricks / storage bricks / coarse lattice points per side
};

// Every limit of the unit in one place.  The largest N is set by the coarse lattice, (nb + 1)^3 <= 2^31 - 1, nb + 1 <= 1290:
// N <= 10313 with B = 8, N <= 5157 with B = 4 (the slot table, nl <= nb + 1, is never larger).
int make_dims(int64_t grid_n, int brick, SparseDims* d) {
    if (!(brick == 4 || brick == 8) || grid_n < 2) return DUDF_E_BADCFG;
    d->m = grid_n - 1; d->shift = brick == 4 ? 2 : 3;
    d->nb = (d->m + brick - 1) / brick; d->nl = d->m / brick + 1; d->ncoarse = d->nb + 1;
    if (d->ncoarse > 1290) return DUDF_E_UNSUPPORTED;
    return 0;
}

// ---- x4 makers: coordinates exactly as make_x4_grid_kernel forms them ----------------------------------------------------------
__device__ __forceinline__ f32x4 grid_x4(int64_t i0, int64_t i1, int64_t i2, int64_t N) {
    const float voxel = 2.0f / (float)(N - 1);
    return f32x4{(float)i0 * voxel - 1.0f, (float)i1 * voxel - 1.0f, (float)i2 * voxel - 1.0f, 1.f};
}

__device__ __forceinline__ int64_t clamp_to(int64_t i, int64_t m) { return i < m ? i : m; }

// lattice point start + c of the nc^3 lattice (first axis slowest) at fine indices min(c_d B, m)
__global__ __launch_bounds__(256) void make_x4_lattice_kernel(float* __restrict__ x4, int64_t n, int64_t np, int64_t N, int64_t nc,
                                                              int B, int64_t start) {
    const int64_t m = N - 1;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < np; c += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = {0, 0, 0, 0};
        if (c < n) {
            const int64_t i = start + c;
            const int64_t c2 = i % nc, c1 = (i / nc) % nc, c0 = i / nc / nc;
            v = grid_x4(clamp_to(c0 * B, m), clamp_to(c1 * B, m), clamp_to(c2 * B, m), N);
        }
        *reinterpret_cast<f32x4*>(x4 + c * 4) = v;
    }
}

// point c of the bricks ids[0 .. n / B^3): brick c / B^3, local (l0, l1, l2) with l2 fastest, global index clamped to m
__global__ __launch_bounds__(256) void make_x4_bricks_kernel(float* __restrict__ x4, int64_t n, int64_t np, int64_t N, int64_t nl,
                                                             int shift, const int32_t* __restrict__ ids) {
    const int64_t m = N - 1;
    const int B = 1 << shift;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < np; c += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = {0, 0, 0, 0};
        if (c < n) {
            const int64_t b = ids[c >> (3 * shift)];
            const int l2 = (int)c & (B - 1), l1 = (int)(c >> shift) & (B - 1), l0 = (int)(c >> (2 * shift)) & (B - 1);
            const int64_t b2 = b % nl, b1 = (b / nl) % nl, b0 = b / nl / nl;
            v = grid_x4(clamp_to(b0 * B + l0, m), clamp_to(b1 * B + l1, m), clamp_to(b2 * B + l2, m), N);
        }
        *reinterpret_cast<f32x4*>(x4 + c * 4) = v;
    }
}

// ---- selection -----------------------------------------------------------------------------------------------------------------
struct SelArgs {
    const float* coarse; double bound;
    int64_t nb, nl, nc, nbricks;                         // nbricks = nl^3
    unsigned char* cand;                                 // [nl^3] candidate flags (pass 1)
    uint32_t* blk; int64_t* off;                         // [nblocks][2] stored / candidate totals and offsets
    int32_t* slot; int32_t* stored; int32_t* cands;      // outputs
};

__global__ __launch_bounds__(DUDF_WG) void sparse_flag_kernel(SelArgs a) {
    const int64_t b = (int64_t)blockIdx.x * DUDF_WG + threadIdx.x;
    if (b >= a.nbricks) return;
    const int64_t b2 = b % a.nl, b1 = (b / a.nl) % a.nl, b0 = b / a.nl / a.nl;
    bool is = false;
    if (b0 < a.nb && b1 < a.nb && b2 < a.nb) {
        float mn = 3.0e38f;
        bool nan = false;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = a.coarse[((b0 + (c & 1)) * a.nc + b1 + ((c >> 1) & 1)) * a.nc + b2 + ((c >> 2) & 1)];
            nan |= !(v == v);
            mn = fminf(mn, v);
        }
        is = nan || (double)mn <= a.bound;
    }
    a.cand[b] = is ? 1 : 0;
}

// stored: the brick itself or one of its up-to-7 lower neighbours b - delta is a candidate
__device__ __forceinline__ void brick_flags(const SelArgs& a, int64_t b, bool& stored, bool& cand) {
    stored = cand = false;
    if (b >= a.nbricks) return;
    const int64_t b2 = b % a.nl, b1 = (b / a.nl) % a.nl, b0 = b / a.nl / a.nl;
    cand = a.cand[b] != 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t q0 = b0 - (c & 1), q1 = b1 - ((c >> 1) & 1), q2 = b2 - ((c >> 2) & 1);
        if (q0 >= 0 && q1 >= 0 && q2 >= 0) stored |= a.cand[(q0 * a.nl + q1) * a.nl + q2] != 0;
    }
}

__global__ __launch_bounds__(DUDF_WG) void sparse_count_kernel(SelArgs a) {
    __shared__ unsigned part[DUDF_WG / 64];
    bool st, cd;
    brick_flags(a, (int64_t)blockIdx.x * DUDF_WG + threadIdx.x, st, cd);
    unsigned ns, nc;
    dudf_wg_rank(st, part, &ns);
    dudf_wg_rank(cd, part, &nc);
    if (threadIdx.x == 0) { a.blk[(int64_t)blockIdx.x * 2] = ns; a.blk[(int64_t)blockIdx.x * 2 + 1] = nc; }
}

__global__ __launch_bounds__(DUDF_WG) void sparse_compact_kernel(SelArgs a) {
    __shared__ unsigned part[DUDF_WG / 64];
    const int64_t b = (int64_t)blockIdx.x * DUDF_WG + threadIdx.x;
    bool st, cd;
    brick_flags(a, b, st, cd);
    unsigned total;
    const unsigned rs = dudf_wg_rank(st, part, &total);
    const unsigned rc = dudf_wg_rank(cd, part, &total);
    if (b >= a.nbricks) return;
    const int64_t os = a.off[(int64_t)blockIdx.x * 2] + rs, oc = a.off[(int64_t)blockIdx.x * 2 + 1] + rc;
    a.slot[b] = st ? (int32_t)os : -1;
    if (st) a.stored[os] = (int32_t)b;
    if (cd) a.cands[oc] = (int32_t)b;
}

size_t carve_select(void* ws, const SparseDims& d, SelArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    const int64_t nbricks = d.nl * d.nl * d.nl, nblocks = (nbricks + DUDF_WG - 1) / DUDF_WG;
    a->off = cv.take<int64_t>(nblocks * 2); a->blk = cv.take<uint32_t>(nblocks * 2); a->cand = cv.take<unsigned char>(nbricks);
    return cv.o;
}

// ---- the CAP-UDF kernels' addressing on brick storage ------------------------------------------------------------------------------
// work item = candidate brick (work >> 3 shift) of the ascending list, cell local (li, lj, lk) with lk fastest: the emission order.
struct BrickAddr {
    const float* df; const float* vec; const int32_t* slot; const int32_t* cands;
    int64_t n_cand, m, nl;
    int shift;
    __device__ __forceinline__ bool locate(int64_t work, int& i, int& j, int& k) const {
        const int64_t q = work >> (3 * shift);
        if (q >= n_cand) return false;
        const int B1 = (1 << shift) - 1;
        const int64_t b = cands[q];
        const int64_t b2 = b % nl, b1 = (b / nl) % nl, b0 = b / nl / nl;
        i = (int)(b0 << shift) + ((int)(work >> (2 * shift)) & B1);
        j = (int)(b1 << shift) + ((int)(work >> shift) & B1);
        k = (int)(b2 << shift) + ((int)work & B1);
        return i < m && j < m && k < m;                  // cells of the last partial brick beyond m are skipped
    }
    // -1: the corner's brick is not stored (a slot table that does not follow the selection rule); the cell then reads a NaN
    __device__ __forceinline__ int64_t corner(int i, int j, int k, int c) const {
        const int B1 = (1 << shift) - 1;
        const int g0 = i + (c & 1), g1 = j + ((c >> 1) & 1), g2 = k + ((c >> 2) & 1);
        const int64_t s = slot[((int64_t)(g0 >> shift) * nl + (g1 >> shift)) * nl + (g2 >> shift)];
        if (s < 0) return -1;
        return ((((((s << shift) + (g0 & B1)) << shift) + (g1 & B1)) << shift) + (g2 & B1));
    }
    __device__ __forceinline__ float value(int64_t p) const { return p < 0 ? __builtin_nanf("") : df[p]; }
    __device__ __forceinline__ const float* vector(int64_t p) const { return vec + p * 3; }
};

struct SparseCapArgs { BrickAddr ad; CapWork w; };

int64_t sparse_cap_blocks(int64_t n_cand, int brick) { return (n_cand * brick * brick * brick + CB - 1) / CB; }

size_t carve_sparse_cap(void* ws, int64_t n_cand, int brick, SparseCapArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    const int64_t nblocks = sparse_cap_blocks(n_cand, brick);
    a->w.off = cv.take<int64_t>(nblocks * 3); a->w.blk = cv.take<uint32_t>(nblocks * 3);
    return cv.o;
}

int sparse_cap_limits(int64_t grid_n, int brick, int64_t n_cand, SparseDims* d) {
    if (int rc = make_dims(grid_n, brick, d)) return rc;
    if (n_cand < 0) return DUDF_E_BADCFG;
    if (n_cand > d->nb * d->nb * d->nb) return DUDF_E_BADCFG;
    if (n_cand * brick * brick * brick > kMaxEntries) return DUDF_E_UNSUPPORTED;
    return 0;
}

int fill_sparse_cap(const float* df, const float* vec, const int32_t* slot, const int32_t* cands, int64_t n_cand, int64_t grid_n,
                    int brick, double threshold, void* ws, size_t bytes, SparseCapArgs* a) {
    SparseDims d;
    if (int rc = sparse_cap_limits(grid_n, brick, n_cand, &d)) return rc;
    if (!df || !vec || !slot || !cands) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(ws, bytes, carve_sparse_cap(ws, n_cand, brick, a))) return rc;
    a->ad = BrickAddr{df, vec, slot, cands, n_cand, d.m, d.nl, d.shift};
    a->w.n = grid_n; a->w.threshold = threshold;
    a->w.verts = nullptr; a->w.tris = nullptr; a->w.cells = nullptr;
    return 0;
}

}  // namespace

extern "C" {

int dudf_grid_fields_lattice(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int brick, int64_t start, int64_t count,
                             int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count, void* workspace,
                             size_t workspace_bytes, void* stream) {
    SparseDims d;
    if (int rc = make_dims(grid_n, brick, &d)) return rc;
    if (start < 0 || count < 0 || start + count > d.ncoarse * d.ncoarse * d.ncoarse || !out_df) return DUDF_E_BADCFG;
    if (!dudf_valid_inverse_mode(inverse_mode)) return DUDF_E_BADMODE;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, count, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (count == 0) return 0;
    {
        DudfProfScope prof(PROF_OTHER, c.st);
        DUDF_TRY(dudf_launch(make_x4_lattice_kernel, dim3(dudf_grid_for(c.lo.np, 256, kGridCap)), dim3(256), c.st, c.ws + c.lo.ws_x4,
                             c.lo.n, c.lo.np, grid_n, d.ncoarse, brick, start));
    }
    if ((rc = dudf_forward_common(c, theta, nullptr, 0, out_vec != nullptr))) return rc;       // value only: no reverse sweep
    return dudf_launch_field_features(c.lo, c.ws, inverse_mode, alpha, out_df, out_vec, out_vec ? out_flag_count : nullptr, nullptr,
                                      nullptr, c.st);
}

size_t dudf_sparse_select_bytes(int64_t grid_n, int brick) {
    SparseDims d;
    if (make_dims(grid_n, brick, &d)) return 0;
    SelArgs a;
    return carve_select(nullptr, d, &a);
}

int dudf_sparse_select(const float* coarse_df, int64_t grid_n, int brick, double bound, int32_t* out_slot, int32_t* out_stored_ids,
                       int32_t* out_candidate_ids, int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
    SparseDims d;
    if (int rc = make_dims(grid_n, brick, &d)) return rc;
    if (!coarse_df || !out_slot || !out_stored_ids || !out_candidate_ids || !out_counts) return DUDF_E_BADCFG;
    SelArgs a;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, carve_select(workspace, d, &a))) return rc;
    a.coarse = coarse_df; a.bound = bound; a.nb = d.nb; a.nl = d.nl; a.nc = d.ncoarse; a.nbricks = d.nl * d.nl * d.nl;
    a.slot = out_slot; a.stored = out_stored_ids; a.cands = out_candidate_ids;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const int64_t nblocks = (a.nbricks + DUDF_WG - 1) / DUDF_WG;
    DUDF_TRY(dudf_launch(sparse_flag_kernel, dim3((unsigned)nblocks), dim3(DUDF_WG), st, a));
    DUDF_TRY(dudf_launch(sparse_count_kernel, dim3((unsigned)nblocks), dim3(DUDF_WG), st, a));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<2>, dim3(1), dim3(1024), st, a.blk, a.off, nblocks, out_counts));
    return dudf_launch(sparse_compact_kernel, dim3((unsigned)nblocks), dim3(DUDF_WG), st, a);
}

int dudf_grid_fields_bricks(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int brick, const int32_t* brick_ids,
                            int64_t n_bricks, int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count,
                            void* workspace, size_t workspace_bytes, void* stream) {
    SparseDims d;
    if (int rc = make_dims(grid_n, brick, &d)) return rc;
    if (n_bricks < 0 || n_bricks > d.nl * d.nl * d.nl || !brick_ids || !out_df || !out_vec) return DUDF_E_BADCFG;
    if (!dudf_valid_inverse_mode(inverse_mode)) return DUDF_E_BADMODE;
    const int64_t count = n_bricks * brick * brick * brick;
    if (count > kMaxEntries) return DUDF_E_UNSUPPORTED;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, count, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (count == 0) return 0;
    {
        DudfProfScope prof(PROF_OTHER, c.st);
        DUDF_TRY(dudf_launch(make_x4_bricks_kernel, dim3(dudf_grid_for(c.lo.np, 256, kGridCap)), dim3(256), c.st, c.ws + c.lo.ws_x4, c.lo.n,
                             c.lo.np, grid_n, d.nl, d.shift, brick_ids));
    }
    if ((rc = dudf_forward_common(c, theta, nullptr, 0, true))) return rc;
    return dudf_launch_field_features(c.lo, c.ws, inverse_mode, alpha, out_df, out_vec, out_flag_count, nullptr, nullptr, c.st);
}

size_t dudf_capudf_sparse_workspace_bytes(int64_t grid_n, int brick, int64_t n_candidates) {
    SparseDims d;
    if (sparse_cap_limits(grid_n, brick, n_candidates, &d)) return 0;
    SparseCapArgs a;
    return carve_sparse_cap(nullptr, n_candidates, brick, &a);
}

int dudf_capudf_sparse_count(const float* df, const float* vec, const int32_t* slot, const int32_t* candidate_ids,
                             int64_t n_candidates, int64_t grid_n, int brick, double threshold, int64_t* out_counts,
                             void* workspace, size_t workspace_bytes, void* stream) {
    SparseCapArgs a;
    int rc = fill_sparse_cap(df, vec, slot, candidate_ids, n_candidates, grid_n, brick, threshold, workspace, workspace_bytes, &a);
    if (rc) return rc;
    if (!out_counts) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const int64_t nblocks = sparse_cap_blocks(n_candidates, brick);
    if (nblocks) DUDF_TRY(dudf_launch(capudf_count_kernel<BrickAddr>, dim3((unsigned)nblocks), dim3(CB), st, a.ad, a.w));
    return dudf_launch(dudf_scan_totals_kernel<3>, dim3(1), dim3(1024), st, a.w.blk, a.w.off, nblocks, out_counts);
}

int dudf_capudf_sparse_emit(const float* df, const float* vec, const int32_t* slot, const int32_t* candidate_ids,
                            int64_t n_candidates, int64_t grid_n, int brick, double threshold, double* out_vertices,
                            int64_t* out_triangles, int64_t* out_cells, void* workspace, size_t workspace_bytes, void* stream) {
    SparseCapArgs a;
    int rc = fill_sparse_cap(df, vec, slot, candidate_ids, n_candidates, grid_n, brick, threshold, workspace, workspace_bytes, &a);
    if (rc) return rc;
    if (!out_vertices || !out_triangles) return DUDF_E_BADCFG;
    a.w.verts = out_vertices; a.w.tris = out_triangles; a.w.cells = out_cells;
    const int64_t nblocks = sparse_cap_blocks(n_candidates, brick);
    if (!nblocks) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(capudf_emit_kernel<BrickAddr>, dim3((unsigned)nblocks), dim3(CB), st, a.ad, a.w);
}

}  // extern "C"
