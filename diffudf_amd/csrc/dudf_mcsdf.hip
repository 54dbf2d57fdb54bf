// Lewiner marching cubes of a SIGNED volume on the GPU — the extraction behind `get_mesh_sdf` (reference src/render_mc.py:314-406,
// which pulls the N^3 grid to the host and calls scikit-image).  Output = the host library's `dudf_mc_lewiner_run`
// (dudf_meshudf.cpp) bit for bit, in the same order: vertices (x, y, z) float32 in grid units, faces int32, raw normal sums, values.
// The cube triangulation (ambiguity tests, 33-case switch) is the shared text of dudf_lewiner.h; this unit is compiled with
// -ffp-contract=off like the host library.
//
// What the serial code does in traversal order is turned into functions of a cell and its neighbours:
//   faces    : raster cell order, then the tiling's triangle order -> exclusive scan of triangle counts over cells.
//   vertices : numbered at first use.  An edge vertex is created by the lowest-raster cell that contains the edge (its OWNER: every
//              tiling uses every crossed edge of its cube, tests/test_mc_lewiner_cpu.py), a centre vertex by its own cell; inside a
//              cell new vertices are numbered by first appearance in its triangle list -> exclusive scan of "owned vertices" over
//              cells, rank inside the owner's list.
//   normals  : the serial code ADDS float contributions in traversal order; the owner walks the <= 4 cells round the edge in raster
//              order, each one's triangle list in order, and performs the same adds in the same sequence (a gather, no atomics).
//   values   : the running maximum of the cubes' value range, taken in the same order.
//
// Mapping: index/compaction work, no matrix cores.  One thread per cell, last axis fastest, 256 cells per workgroup.
//   pass 1 classify : 8 corner reads per cell (neighbouring rows hit L1/L2), sign mask -> CASES (512 B staged in LDS).  The active
//                     cells of the workgroup (a thin shell) are compacted in LDS so that the divergent 33-case switch runs in full
//                     waves; only workgroups that have any stage the other tables (17 KB) in LDS.  Per cell one 32-bit word
//                     (tiling, configuration, in-workgroup vertex prefix; 0 = nothing) for pass 3 and for the neighbours; per
//                     workgroup the vertex / triangle totals.
//   pass 2 scan     : exclusive scan of the workgroup totals (dudf_scan_totals_kernel<2>: one workgroup), totals -> out_counts.
//   pass 3 emit     : active cells compacted again; faces through the owners' words, vertices / normals / values by their owners.
// The table descriptors (offsets, dimensions) travel as kernel arguments and are staged in LDS beside the table bytes, as LDS
// pointers: a look-up whose table is chosen per lane (the tiling) is two DS reads, none through a flat address.
#include "dudf_context.h"
#include "dudf_wgscan.h"
#include "dudf_lewiner.h"

namespace {

using namespace dudf_lewiner;

constexpr int CB = DUDF_WG;                              // cells per workgroup
constexpr int kLutCap = 18 * 1024;                       // bytes of LDS for the caller's tables (the standard set: 17 548)

struct LutDesc { int off[N_LUTS]; short l1[N_LUTS], l2[N_LUTS]; int total; };

struct McArgs {
    const float* im; const int8_t* luts; LutDesc d;
    int64_t ny, nx;                                      // grid points along axes 1, 2
    int64_t cy, cx, ncells;                              // cells along axes 1, 2; all cells
    int cz;
    double level;
    uint32_t* word;                                      // [ncells]
    uint32_t* blk;                                       // [nblocks][2] vertex / triangle totals (pass 1)
    int64_t* off;                                        // [nblocks][2] exclusive offsets (pass 2)
    float* verts; int* faces; float* normals; float* values;
};

// word: lut 0-5 | sub + 2 6-9 | nt 10-13 | config 14-19 | vertices created by earlier cells of the workgroup 20-31 (<= 255 * 13)
__device__ __forceinline__ uint32_t pack_word(const Tiling& t, int config, unsigned prefix) {
    return (uint32_t)t.lut | ((uint32_t)(t.sub + 2) << 6) | ((uint32_t)t.nt << 10) | ((uint32_t)config << 14) | (prefix << 20);
}
__device__ __forceinline__ Tiling word_tiling(uint32_t w) { return Tiling{(int)(w & 63), (int)((w >> 6) & 15) - 2, (int)((w >> 10) & 15)}; }
__device__ __forceinline__ int word_config(uint32_t w) { return (int)((w >> 14) & 63); }

struct Cell { int z, y, x; };
__device__ __forceinline__ Cell cell_of(const McArgs& a, int64_t cell) {
    const int64_t x = cell % a.cx, zy = cell / a.cx;
    return Cell{(int)(zy / a.cy), (int)(zy % a.cy), (int)x};
}
__device__ __forceinline__ int64_t cell_id(const McArgs& a, int z, int y, int x) { return ((int64_t)z * a.cy + y) * a.cx + x; }

// corner value at the grid point (dx, dy, dz) of a cell, as the host forms it
__device__ __forceinline__ double cval(const McArgs& a, const Cell& c, int dx, int dy, int dz) {
    return (double)a.im[((int64_t)(c.z + dz) * a.ny + (c.y + dy)) * a.nx + (c.x + dx)] - a.level;
}
// cube numbering of the tables: corner c sits at (kDx, kDy, kDz)
__device__ __forceinline__ int cdx(int c) { return ((c + 1) >> 1) & 1; }
__device__ __forceinline__ int cdy(int c) { return (c >> 1) & 1; }
__device__ __forceinline__ int cdz(int c) { return (c >> 2) & 1; }
__device__ __forceinline__ int cidx(int dx, int dy, int dz) { return dz * 4 + (dy ? (dx ? 2 : 3) : dx); }

// Edge geometry as `Mesher::slot` has it: edges 0/2/4/6 run along x, 1/3/5/7 along y, 8-11 along z; lo = the edge's lower grid point.
__device__ __forceinline__ int edge_axis(int e) { return e >= 8 ? 2 : (e & 1); }
__device__ __forceinline__ void edge_lo(int e, int& dx, int& dy, int& dz) {
    if (e < 8) { dz = e >> 2; const int r = e & 3; dx = r == 1; dy = r == 2; }
    else { dz = 0; dx = e == 9 || e == 10; dy = e >= 10; }
}
__device__ __forceinline__ int edge_id(int axis, int dx, int dy, int dz) {
    if (axis == 0) return 2 * dy + 4 * dz;
    if (axis == 1) return (dx ? 1 : 3) + 4 * dz;
    return 8 + (dy ? (dx ? 2 : 3) : dx);
}
// the cell creates the vertex of its edge e: it is the lowest-raster cell round that edge (the centre vertex, 12, is its own)
__device__ __forceinline__ bool owns(const Cell& c, int e) {
    if (e >= 12) return true;
    int dx, dy, dz; edge_lo(e, dx, dy, dz);
    const int ax = edge_axis(e);
    return (ax == 0 || dx || c.x == 0) && (ax == 1 || dy || c.y == 0) && (ax == 2 || dz || c.z == 0);
}
__device__ __forceinline__ Cell owner_of(const Cell& c, int e, int& e_owner) {
    if (e >= 12) { e_owner = 12; return c; }
    int dx, dy, dz; edge_lo(e, dx, dy, dz);
    const int ax = edge_axis(e);
    Cell o = c;
    if (ax != 0) { const int p = c.x + dx; o.x = p > 0 ? p - 1 : 0; dx = p - o.x; } else dx = 0;
    if (ax != 1) { const int p = c.y + dy; o.y = p > 0 ? p - 1 : 0; dy = p - o.y; } else dy = 0;
    if (ax != 2) { const int p = c.z + dz; o.z = p > 0 ? p - 1 : 0; dz = p - o.z; } else dz = 0;
    e_owner = edge_id(ax, dx, dy, dz);
    return o;
}

// position of edge e among the vertices its cell creates, in first-appearance order of the cell's triangle list
__device__ int rank_in(const Lut* L, uint32_t w, const Cell& c, int e) {
    const Tiling t = word_tiling(w);
    const int config = word_config(w);
    unsigned seen = 0;
    int n = 0;
    for (int k = 0; k < 3 * t.nt; ++k) {
        const int ek = edge_of(L, t, config, k) & 15;
        if (seen >> ek & 1) continue;
        seen |= 1u << ek;
        if (ek == e) return n;
        n += owns(c, ek) ? 1 : 0;
    }
    return n;
}
__device__ int appearances(const Lut* L, uint32_t w, int e) {
    const Tiling t = word_tiling(w);
    const int config = word_config(w);
    int n = 0;
    for (int k = 0; k < 3 * t.nt; ++k) n += (edge_of(L, t, config, k) & 15) == e ? 1 : 0;
    return n;
}

// ---- LDS staging --------------------------------------------------------------------------------------------------------------
struct Tables { int8_t data[kLutCap]; Lut lut[N_LUTS]; };

__device__ __forceinline__ void stage_descriptors(const McArgs& a, Tables& T) {
    if (threadIdx.x < N_LUTS) {
        const int i = threadIdx.x;
        T.lut[i].v = (const DUDF_LW_TABLE int8_t*)T.data + a.d.off[i]; T.lut[i].l1 = a.d.l1[i]; T.lut[i].l2 = a.d.l2[i];
    }
}
__device__ __forceinline__ void stage_bytes(const McArgs& a, Tables& T, int from, int to) {       // bytes [from, to) of the tables
    const int f4 = (from + 3) & ~3, t4 = to & ~3;
    if (t4 <= f4) {
        for (int i = from + threadIdx.x; i < to; i += CB) T.data[i] = a.luts[i];
        return;
    }
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.luts);
    uint32_t* dst = reinterpret_cast<uint32_t*>(T.data);
    for (int i = f4 / 4 + threadIdx.x; i < t4 / 4; i += CB) dst[i] = src[i];
    if ((int)threadIdx.x < f4 - from) T.data[from + threadIdx.x] = a.luts[from + threadIdx.x];
    if ((int)threadIdx.x < to - t4) T.data[t4 + threadIdx.x] = a.luts[t4 + threadIdx.x];
}

// the eight corner values of the cell a thread works on, one column of LDS per thread (dynamic corner indices without scratch)
struct CornerView {
    const double* p;
    __device__ __forceinline__ double operator[](int i) const { return p[i * CB]; }
};

// compaction of the workgroup's active cells: list[rank] = thread, returns the number of active cells
__device__ __forceinline__ int compact_active(bool active, unsigned short* list, unsigned* wave_tot) {
    unsigned total;
    const unsigned rank = dudf_wg_rank(active, wave_tot, &total);
    if (active) list[rank] = (unsigned short)threadIdx.x;
    __syncthreads();
    return (int)total;
}

__global__ __launch_bounds__(CB) void mc_classify_kernel(McArgs a) {
    __shared__ Tables T;
    __shared__ double sv[8 * CB];
    __shared__ uint32_t sword[CB];
    __shared__ unsigned short list[CB];
    __shared__ unsigned wave_tot[CB / 64];
    const int tid = threadIdx.x;
    const int64_t cell0 = (int64_t)blockIdx.x * CB, cell = cell0 + tid;
    stage_descriptors(a, T);
    stage_bytes(a, T, a.d.off[CASES], a.d.off[CASES] + 512);
    sword[tid] = 0;
    __syncthreads();
    bool active = false;
    if (cell < a.ncells) {
        const Cell c = cell_of(a, cell);
        int index = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) index |= cval(a, c, cdx(q), cdy(q), cdz(q)) > 0.0 ? 1 << q : 0;
        active = T.lut[CASES].at(index, 0) > 0;
    }
    const int nact = compact_active(active, list, wave_tot);
    if (nact == 0) {                                     // (uniform) nothing crosses this workgroup's cells
        if (cell < a.ncells) a.word[cell] = 0;
        if (tid == 0) { a.blk[(int64_t)blockIdx.x * 2] = 0; a.blk[(int64_t)blockIdx.x * 2 + 1] = 0; }
        return;
    }
    stage_bytes(a, T, 0, a.d.total);
    __syncthreads();
    Tiling t = {TILING1, -1, 0};
    int config = 0, lid = 0;
    unsigned nv = 0;
    if (tid < nact) {
        lid = list[tid];
        const Cell c = cell_of(a, cell0 + lid);
        int index = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double v = cval(a, c, cdx(q), cdy(q), cdz(q));
            sv[q * CB + tid] = v;
            index |= v > 0.0 ? 1 << q : 0;
        }
        config = T.lut[CASES].at(index, 1);
        t = resolve(CornerView{sv + tid}, T.lut, T.lut[CASES].at(index, 0), config);
        unsigned seen = 0;
        for (int k = 0; k < 3 * t.nt; ++k) {
            const int e = edge_of(T.lut, t, config, k) & 15;
            if (!(seen >> e & 1)) nv += owns(c, e) ? 1 : 0;
            seen |= 1u << e;
        }
    }
    unsigned tv, tt;
    const unsigned prefix = dudf_wg_scan(nv, wave_tot, &tv);      // compacted order = raster order
    dudf_wg_scan((unsigned)t.nt, wave_tot, &tt);
    if (tid < nact) sword[lid] = pack_word(t, config, prefix);
    __syncthreads();
    if (cell < a.ncells) a.word[cell] = sword[tid];
    if (tid == 0) { a.blk[(int64_t)blockIdx.x * 2] = tv; a.blk[(int64_t)blockIdx.x * 2 + 1] = tt; }
}

__device__ __forceinline__ int64_t vertex_base(const McArgs& a, int64_t cell, uint32_t w) { return a.off[(cell / CB) * 2] + (w >> 20); }

// The vertex of edge e (< 12) of cell c, which creates it: position as `corner_of_triangle` computes it for the first user, normal
// sum and value gathered over the cells round the edge in the order the serial code visits them.
__device__ void emit_edge_vertex(const McArgs& a, const Lut* L, const Cell& c, int e, int64_t vi) {
    const int dx1 = L[EDGESRELX].at(e, 0), dx2 = L[EDGESRELX].at(e, 1);
    const int dy1 = L[EDGESRELY].at(e, 0), dy2 = L[EDGESRELY].at(e, 1);
    const int dz1 = L[EDGESRELZ].at(e, 0), dz2 = L[EDGESRELZ].at(e, 1);
    {
        const double w1 = 1.0 / (kEps + fabs(cval(a, c, dx1, dy1, dz1))), w2 = 1.0 / (kEps + fabs(cval(a, c, dx2, dy2, dz2)));
        double fx = 0.0, fy = 0.0, fz = 0.0, ff = 0.0;
        fx += (double)dx1 * w1; fy += (double)dy1 * w1; fz += (double)dz1 * w1; ff += w1;
        fx += (double)dx2 * w2; fy += (double)dy2 * w2; fz += (double)dz2 * w2; ff += w2;
        a.verts[vi * 3] = (float)((double)c.x + 1.0 * fx / ff);
        a.verts[vi * 3 + 1] = (float)((double)c.y + 1.0 * fy / ff);
        a.verts[vi * 3 + 2] = (float)((double)c.z + 1.0 * fz / ff);
    }
    int lx, ly, lz; edge_lo(e, lx, ly, lz);
    const int ax = edge_axis(e);
    const int px = c.x + lx, py = c.y + ly, pz = c.z + lz;           // the edge's lower grid point
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, val = 0.f;
    for (int qz = (ax == 2 ? 0 : -1); qz <= 0; ++qz)
        for (int qy = (ax == 1 ? 0 : -1); qy <= 0; ++qy)
            for (int qx = (ax == 0 ? 0 : -1); qx <= 0; ++qx) {
                const Cell q = {pz + qz, py + qy, px + qx};
                if (q.z < 0 || q.y < 0 || q.x < 0 || q.z >= a.cz || q.y >= a.cy || q.x >= a.cx) continue;
                const uint32_t w = a.word[cell_id(a, q.z, q.y, q.x)];
                const int eq = edge_id(ax, -qx, -qy, -qz);
                const int k = w ? appearances(L, w, eq) : 0;
                if (k == 0) continue;
                // this cube's `prepare()`: value range, and the gradients at the two table corners of its edge
                double hi = 0.0, lo = 0.0;
#pragma unroll
                for (int i = 0; i < 8; ++i) { const double v = cval(a, q, i & 1, (i >> 1) & 1, i >> 2); hi = v > hi ? v : hi; lo = v < lo ? v : lo; }
                const double vmax = hi - lo;
                if (vmax > val) val = (float)vmax;
                const int ex1 = L[EDGESRELX].at(eq, 0), ex2 = L[EDGESRELX].at(eq, 1);
                const int ey1 = L[EDGESRELY].at(eq, 0), ey2 = L[EDGESRELY].at(eq, 1);
                const int ez1 = L[EDGESRELZ].at(eq, 0), ez2 = L[EDGESRELZ].at(eq, 1);
                const float w1 = (float)(1.0 / (kEps + fabs(cval(a, q, ex1, ey1, ez1))));
                const float w2 = (float)(1.0 / (kEps + fabs(cval(a, q, ex2, ey2, ez2))));
                float g[2][3];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    // `vg_[i]` with i = dz 4 + dy 2 + dx is the gradient at the table's corner NUMBER i (as the reference indexes it)
                    const int i = s ? ez2 * 4 + ey2 * 2 + ex2 : ez1 * 4 + ey1 * 2 + ex1;
                    const int X = cdx(i), Y = cdy(i), Z = cdz(i);
                    const float ws = s ? w2 : w1;
                    g[s][0] = (float)((cval(a, q, 0, Y, Z) - cval(a, q, 1, Y, Z)) * ws);
                    g[s][1] = (float)((cval(a, q, X, 0, Z) - cval(a, q, X, 1, Z)) * ws);
                    g[s][2] = (float)((cval(a, q, X, Y, 0) - cval(a, q, X, Y, 1)) * ws);
                }
                for (int r = 0; r < k; ++r) {
                    n0 += g[0][0]; n1 += g[0][1]; n2 += g[0][2];
                    n0 += g[1][0]; n1 += g[1][1]; n2 += g[1][2];
                }
            }
    a.normals[vi * 3] = n0; a.normals[vi * 3 + 1] = n1; a.normals[vi * 3 + 2] = n2;
    a.values[vi] = val;
}

// The centre vertex of the cell whose corner values are `v` (`calculate_center_vertex`, with the reference's quirk: the z sum goes
// to the x component, the z component stays 0); it is used `k` times, by this cell only.
__device__ void emit_centre_vertex(const McArgs& a, const Cell& c, const CornerView& v, int k, int64_t vi) {
    double w[8], fx = 0.0, fy = 0.0, fz = 0.0, ff = 0.0, hi = 0.0, lo = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const double x = v[i]; w[i] = 1.0 / (kEps + fabs(x)); hi = x > hi ? x : hi; lo = x < lo ? x : lo; }
#pragma unroll
    for (int i = 0; i < 8; ++i) { fx += (double)cdx(i) * w[i]; fy += (double)cdy(i) * w[i]; fz += (double)cdz(i) * w[i]; ff += w[i]; }
    a.verts[vi * 3] = (float)(c.x + 1.0 * fx / ff);
    a.verts[vi * 3 + 1] = (float)(c.y + 1.0 * fy / ff);
    a.verts[vi * 3 + 2] = (float)(c.z + 1.0 * fz / ff);
    double gy = 0.0, gz = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) gy += w[i] * (v[cidx(cdx(i), 0, cdz(i))] - v[cidx(cdx(i), 1, cdz(i))]);
#pragma unroll
    for (int i = 0; i < 8; ++i) gz += w[i] * (v[cidx(cdx(i), cdy(i), 0)] - v[cidx(cdx(i), cdy(i), 1)]);
    float n0 = 0.f, n1 = 0.f;
    for (int r = 0; r < k; ++r) { n0 += (float)gz; n1 += (float)gy; }
    a.normals[vi * 3] = n0; a.normals[vi * 3 + 1] = n1; a.normals[vi * 3 + 2] = 0.f;
    const double vmax = hi - lo;
    a.values[vi] = vmax > 0.0 ? (float)vmax : 0.f;
}

__global__ __launch_bounds__(CB) void mc_emit_kernel(McArgs a) {
    __shared__ Tables T;
    __shared__ double sv[8 * CB];
    __shared__ unsigned short list[CB];
    __shared__ unsigned wave_tot[CB / 64];
    const int tid = threadIdx.x;
    const int64_t cell0 = (int64_t)blockIdx.x * CB, cell = cell0 + tid;
    const bool active = cell < a.ncells && a.word[cell] != 0;
    const int nact = compact_active(active, list, wave_tot);
    if (nact == 0) return;                               // (uniform)
    stage_descriptors(a, T);
    stage_bytes(a, T, 0, a.d.total);
    __syncthreads();
    const bool mine = tid < nact;
    const int64_t me = mine ? cell0 + list[tid] : 0;
    const uint32_t w = mine ? a.word[me] : 0;
    const Tiling t = word_tiling(w);
    unsigned tt;
    const unsigned tpre = dudf_wg_scan(mine ? (unsigned)t.nt : 0u, wave_tot, &tt);
    if (!mine) return;
    const Cell c = cell_of(a, me);
    const int config = word_config(w);
    const int64_t v0 = vertex_base(a, me, w);
    int* faces = a.faces + (a.off[(int64_t)blockIdx.x * 2 + 1] + tpre) * 3;
    unsigned seen = 0;
    int created = 0;
    for (int k = 0; k < 3 * t.nt; ++k) {
        const int e = edge_of(T.lut, t, config, k) & 15;
        int eo;
        const Cell o = owner_of(c, e, eo);
        const bool self = o.z == c.z && o.y == c.y && o.x == c.x;
        int64_t vi;
        if (self) {
            if (!(seen >> e & 1)) {                       // first use: this cell creates the vertex
                vi = v0 + created++;
                if (e < 12) emit_edge_vertex(a, T.lut, c, e, vi);
                else {
#pragma unroll
                    for (int q = 0; q < 8; ++q) sv[q * CB + tid] = cval(a, c, cdx(q), cdy(q), cdz(q));
                    emit_centre_vertex(a, c, CornerView{sv + tid}, appearances(T.lut, w, 12), vi);
                }
            } else vi = v0 + rank_in(T.lut, w, c, e);
        } else {
            const int64_t oc = cell_id(a, o.z, o.y, o.x);
            const uint32_t ow = a.word[oc];
            vi = vertex_base(a, oc, ow) + rank_in(T.lut, ow, o, eo);
        }
        seen |= 1u << e;
        faces[k] = (int)vi;
    }
}

int64_t mc_blocks(int64_t nz, int64_t ny, int64_t nx) { return ((nz - 1) * (ny - 1) * (nx - 1) + CB - 1) / CB; }
bool mc_dims_ok(int64_t nz, int64_t ny, int64_t nx) { return nz >= 2 && ny >= 2 && nx >= 2 && nz <= 2048 && ny <= 2048 && nx <= 2048; }

// the one statement of the workspace's layout: sizes with a null base, places on the caller's
size_t carve_mc(void* ws, int64_t nz, int64_t ny, int64_t nx, McArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    const int64_t nb = mc_blocks(nz, ny, nx);
    a->off = cv.take<int64_t>(nb * 2); a->blk = cv.take<uint32_t>(nb * 2); a->word = cv.take<uint32_t>((nz - 1) * (ny - 1) * (nx - 1));
    return cv.o;
}

int fill_args(const float* volume, int64_t nz, int64_t ny, int64_t nx, double level, const signed char* luts, const int64_t* offs,
              const int32_t* dims, int n_luts, void* ws, size_t bytes, McArgs* a) {
    if (!mc_dims_ok(nz, ny, nx) || !volume || !luts || !offs || !dims || n_luts != N_LUTS) return DUDF_E_BADCFG;
    if (reinterpret_cast<uintptr_t>(luts) & 3) return DUDF_E_BADCFG;
    int64_t total = 0;
    for (int i = 0; i < N_LUTS; ++i) {                   // tables inside the staged bytes, dimensions that fit the descriptor
        const int64_t d0 = dims[3 * i], d1 = dims[3 * i + 1], d2 = dims[3 * i + 2];
        if (d0 < 1 || d1 < 1 || d2 < 1 || d0 > 4096 || d1 > 4096 || d2 > 4096 || offs[i] < 0 || offs[i] > kLutCap) return DUDF_E_BADCFG;
        const int64_t end = offs[i] + d0 * d1 * d2;
        if (end > kLutCap) return DUDF_E_BADCFG;
        total = end > total ? end : total;
        a->d.off[i] = (int)offs[i]; a->d.l1[i] = (short)d1; a->d.l2[i] = (short)d2;
    }
    if (dims[3 * CASES] * dims[3 * CASES + 1] < 512 || dims[3 * EDGESRELX] * dims[3 * EDGESRELX + 1] < 24 ||
        dims[3 * EDGESRELY] * dims[3 * EDGESRELY + 1] < 24 || dims[3 * EDGESRELZ] * dims[3 * EDGESRELZ + 1] < 24) return DUDF_E_BADCFG;
    a->d.total = (int)total;
    if (int rc = dudf_check_buffer(ws, bytes, carve_mc(ws, nz, ny, nx, a))) return rc;
    a->im = volume; a->luts = reinterpret_cast<const int8_t*>(luts);
    a->ny = ny; a->nx = nx; a->cz = (int)(nz - 1); a->cy = ny - 1; a->cx = nx - 1; a->ncells = (nz - 1) * (ny - 1) * (nx - 1);
    a->level = level;
    a->verts = nullptr; a->faces = nullptr; a->normals = nullptr; a->values = nullptr;
    return 0;
}

}  // namespace

extern "C" {

size_t dudf_mc_lewiner_workspace_bytes(int64_t nz, int64_t ny, int64_t nx) {
    if (!mc_dims_ok(nz, ny, nx)) return 0;
    McArgs a;
    return carve_mc(nullptr, nz, ny, nx, &a);
}

int dudf_mc_lewiner_count(const float* volume, int64_t nz, int64_t ny, int64_t nx, double level, const signed char* luts,
                          const int64_t* lut_offsets, const int32_t* lut_dims, int n_luts, int64_t* out_counts, void* workspace,
                          size_t workspace_bytes, void* stream) {
    McArgs a;
    int rc = fill_args(volume, nz, ny, nx, level, luts, lut_offsets, lut_dims, n_luts, workspace, workspace_bytes, &a);
    if (rc) return rc;
    if (!out_counts) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const int64_t nb = mc_blocks(nz, ny, nx);
    DUDF_TRY(dudf_launch(mc_classify_kernel, dim3((unsigned)nb), dim3(CB), st, a));
    return dudf_launch(dudf_scan_totals_kernel<2>, dim3(1), dim3(1024), st, a.blk, a.off, nb, out_counts);
}

int dudf_mc_lewiner_emit(const float* volume, int64_t nz, int64_t ny, int64_t nx, double level, const signed char* luts,
                         const int64_t* lut_offsets, const int32_t* lut_dims, int n_luts, float* out_vertices, int32_t* out_faces,
                         float* out_normals, float* out_values, void* workspace, size_t workspace_bytes, void* stream) {
    McArgs a;
    int rc = fill_args(volume, nz, ny, nx, level, luts, lut_offsets, lut_dims, n_luts, workspace, workspace_bytes, &a);
    if (rc) return rc;
    if (!out_vertices || !out_faces || !out_normals || !out_values) return DUDF_E_BADCFG;
    a.verts = out_vertices; a.faces = out_faces; a.normals = out_normals; a.values = out_values;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(mc_emit_kernel, dim3((unsigned)mc_blocks(nz, ny, nx)), dim3(CB), st, a);
}

}  // extern "C"
