// The per-cell CAP-UDF evaluation and its two kernels, written once over an ADDRESSING POLICY: where a work item's cell lies in the
// grid and where its 8 corners lie in the arrays.  dudf_capudf.hip instantiates it on the dense (N,N,N) arrays, dudf_sparsegrid.hip
// on brick storage behind a slot table; the active test, the sign rule, the table, the interpolation and the vertex formula are
// these lines for both, which is what lets the sparse extraction be compared with the dense one bit for bit.
// Internal: device code only, not installed, nothing here is part of the C ABI.
//
// A policy A provides
//   bool    locate(int64_t work, int& i, int& j, int& k)   the GLOBAL cell index of work item `work`; false: no cell there
//   int64_t corner(int i, int j, int k, int c)             the position of corner c = ii + 2 jj + 4 kk of that cell in ndf / grad
//   float   value(int64_t p)                               ndf at such a position
//   const float* vector(int64_t p)                         the 3 floats of grad at such a position (only asked for a cell that
//                                                          passed the active test)
#pragma once
#include "dudf_wgscan.h"

namespace {

#define DUDF_MC_QUAL __constant__ const
#include "dudf_mc_table.h"          // kMcEdgeMask[256], kMcTri[256][1 + 3 * DUDF_MC_MAX_TRI], kMcEdgeCorner[12][2]

constexpr int CB = DUDF_WG;                              // cells per workgroup

struct CapWork {
    int64_t n;                                           // grid points per side: the vertex formula's N
    double threshold;
    uint32_t* blk;                                       // [nblocks][3] totals (pass 1)
    int64_t* off;                                        // [nblocks][3] exclusive offsets (pass 2)
    double* verts; int64_t* tris; int64_t* cells;        // outputs (pass 3)
};

struct CellEval { int idx; float res[8]; int i, j, k; };

// case index of a cell (0 = nothing to emit) and its signed corner values
template <class A>
__device__ __forceinline__ bool eval_cell(const A& ad, const CapWork& a, int64_t work, CellEval& ce) {
#pragma clang fp contract(off)                                   // the dot product below: products rounded, then added
    ce.idx = 0;
    if (!ad.locate(work, ce.i, ce.j, ce.k)) return false;
    float v[8];
    float mn = 3.0e38f;
    bool nan = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = ad.value(ad.corner(ce.i, ce.j, ce.k, c));
        nan |= !(v[c] == v[c]);
        mn = fminf(mn, v[c]);
    }
    if (nan || (double)mn > a.threshold) return false;   // np.min(ndf_loc) > threshold: continue (float64 comparison)
    const float* g0 = ad.vector(ad.corner(ce.i, ce.j, ce.k, 0));
    const float gx = g0[0], gy = g0[1], gz = g0[2];
    int idx = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float* g = ad.vector(ad.corner(ce.i, ce.j, ce.k, c));
        const float d = __fadd_rn(__fadd_rn(__fmul_rn(gx, g[0]), __fmul_rn(gy, g[1])), __fmul_rn(gz, g[2]));
        const float r = d < 0.f ? -v[c] : v[c];
        ce.res[c] = r;
        idx |= (r < 0.f) ? (1 << c) : 0;
    }
    ce.idx = idx;
    return idx != 0;                                      // res.min() < 0
}

__device__ __forceinline__ unsigned pack_counts(int idx) {    // cells | vertices << 9 | triangles << 21
    if (!idx) return 0u;
    return 1u | ((unsigned)__popc((unsigned)kMcEdgeMask[idx]) << 9) | ((unsigned)kMcTri[idx][0] << 21);
}

template <class A>
__global__ __launch_bounds__(CB) void capudf_count_kernel(A ad, CapWork a) {
    __shared__ unsigned part[CB / 64];
    const int64_t work = (int64_t)blockIdx.x * CB + threadIdx.x;
    CellEval ce;
    unsigned w = 0;
    if (eval_cell(ad, a, work, ce)) w = pack_counts(ce.idx);
    unsigned nc = w & 0x1ff, nv = (w >> 9) & 0xfff, nt = w >> 21;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nc += __shfl_xor(nc, o); nv += __shfl_xor(nv, o); nt += __shfl_xor(nt, o); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) part[wave] = nc | (nv << 9) | (nt << 21);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0, v = 0, t = 0;
        for (int q = 0; q < CB / 64; ++q) { c += part[q] & 0x1ff; v += (part[q] >> 9) & 0xfff; t += part[q] >> 21; }
        a.blk[(int64_t)blockIdx.x * 3] = c; a.blk[(int64_t)blockIdx.x * 3 + 1] = v; a.blk[(int64_t)blockIdx.x * 3 + 2] = t;
    }
}

template <class A>
__global__ __launch_bounds__(CB) void capudf_emit_kernel(A ad, CapWork a) {
    __shared__ unsigned part[CB / 64];
    const int64_t work = (int64_t)blockIdx.x * CB + threadIdx.x;
    CellEval ce;
    unsigned w = 0;
    const bool live = eval_cell(ad, a, work, ce);
    if (live) w = pack_counts(ce.idx);
    // exclusive scan of the three packed counts over the workgroup: one word, no field can carry into the next (<= 256 / 3072 / 1280).
    // The shared helper's total is not needed here (the compiler drops it) and its leading barrier is one more than a private scan
    // of words nobody else uses would need: the price of ONE scan for all extraction kernels.  The extraction's time stays inside
    // the parent's run-to-run spread (profiles/HISTORY.md).
    unsigned total;
    const unsigned exc = dudf_wg_scan(w, part, &total);
    if (!live) return;
    const int64_t* o3 = a.off + (int64_t)blockIdx.x * 3;
    const int64_t c0 = o3[0] + (exc & 0x1ff), v0 = o3[1] + ((exc >> 9) & 0xfff), t0 = o3[2] + (exc >> 21);
    if (a.cells) { a.cells[c0 * 3] = ce.i; a.cells[c0 * 3 + 1] = ce.j; a.cells[c0 * 3 + 2] = ce.k; }
    const unsigned mask = kMcEdgeMask[ce.idx];
    const double inv = (double)(a.n - 1);
    const double org[3] = {(double)ce.i, (double)ce.j, (double)ce.k};
    int slot[12];
    int nvert = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        slot[e] = nvert;
        if (mask >> e & 1) {
            const int ca = kMcEdgeCorner[e][0], cb = kMcEdgeCorner[e][1];
            const double va = (double)ce.res[ca], vb = (double)ce.res[cb];
            const double t = va / (va - vb);
            const int axis = e >> 2;                      // edges 0-3 run along axis 0, 4-7 along 1, 8-11 along 2
            double* out = a.verts + (v0 + nvert) * 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double local = (d == axis) ? t : (double)((ca >> d) & 1);
                out[d] = (local + org[d]) / inv * 2.0 - 1.0;
            }
            ++nvert;
        }
    }
    const int ntri = kMcTri[ce.idx][0];
    for (int q = 0; q < ntri; ++q)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int e = kMcTri[ce.idx][1 + 3 * q + d];
            int sl = 0;
#pragma unroll
            for (int x = 0; x < 12; ++x) sl = (x == e) ? slot[x] : sl;
            a.tris[(t0 + q) * 3 + d] = v0 + sl;
        }
}

}  // namespace
