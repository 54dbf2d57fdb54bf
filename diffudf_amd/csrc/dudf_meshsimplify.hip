// Mesh simplification on the device: quadric vertex clustering on a uniform lattice (Lindstrom's one-pass out-of-core simplification)
// with border quadrics, the last link of weld -> wind -> drop floaters -> simplify.  The rules are DESIGN.md §3.6c;
// tests/simplify_oracle.py restates them in numpy.  Built with -ffp-contract=off: every sum repeats the oracle's brackets in fp64.
// Index work, one thread per item; integer atomics on hash-table slots and counters, no float atomics: a cell's quadric is summed by
// ONE thread that walks the cell's run of records in (key, face) order, so the order of the additions is part of the result.
//
// Three calls around one sort.  `_keys` validates the faces, enters the valid faces' edges into the edge table and writes one key per
// face corner (a corner that does not contribute a record gets -1, which sorts first); the caller sorts the keys stably and hands the
// sorted keys and the permutation to `_count`, which finds the occupied cells (heads of the runs), remaps and prunes the faces, sums and
// places every cell and publishes the eight counts; `_emit` compacts the used cells and the surviving faces.
//
// Hash tables, by the rules of dudf_meshtab.h:
//   edges   capacity >= 6 F, beside a slot the use count;
//   faces   smallest face index per sorted triple of cell ids (read from `g`, which the launch before wrote), capacity >= 2 F.
#include "dudf_meshtab.h"
#include "dudf_eigh3.h"

namespace {

constexpr int WG = DUDF_WG;
constexpr int64_t KEY_NONE = -1;                               // a corner without a record: sorts in front of every cell (the
                                                               // all-saturated cell's key is 2^63 - 1: nothing sorts behind it)
constexpr int64_t CELL_MASK = (1ll << 21) - 1;
constexpr int64_t MAGIC_SIMPLIFY = 0x6475646653314d50ll;
enum { ST_INVALID = 0, ST_REPEATED = 1, ST_VALID = 2, ST_COLLAPSED = 3, ST_DUPLICATE = 4, ST_ALIVE = 5 };
enum { CTR_INVALID = 0, CTR_COLLAPSED, CTR_DUPLICATE, CTR_BORDER, CTR_FALLBACK, N_CTR };
enum { TOT_CELLS = 0, TOT_USED, TOT_FACES, N_TOT };
enum { HEAD_MAGIC = 0, HEAD_V, HEAD_F, HEAD_PLACED, N_HEAD };

struct SimpArgs {
    const double* vert; const int64_t* face; int64_t V, F, capE, capF, Cmax, nbS, nbF, nbC;
    double org[3]; double h, inv, wb, tau;
    const int64_t* skey; const int64_t* perm;       // [3 F] the sorted corner keys and the corner each came from
    int64_t* head;                       // [N_HEAD] magic, V, F, placed: what the workspace holds (emit checks it on the device)
    int64_t* tot;                        // [N_TOT] occupied cells, used cells, surviving faces
    unsigned long long* ctr;             // [N_CTR]
    uint32_t* ecnt;                      // [capE] uses of the edge
    uint8_t* cuse;                       // [Cmax] a surviving face uses the cell
    unsigned long long* etab;            // [capE] edge keys
    uint32_t* ftab;                      // [capF] smallest face index of a cell triple
    int32_t* g;                          // [3 F] cell id of a corner, -1 until known
    uint8_t* fstate;                     // [F] ST_*
    uint8_t* fborder;                    // [F] bit k: edge k (corner k -> k + 1) is a border edge
    uint8_t* first;                      // [3 F] the first corner of the face with this corner's key
    int32_t* cstart;                     // [Cmax] first record of the cell in the sorted order
    int64_t* ckey;                       // [Cmax]
    int32_t* ccount;                     // [Cmax] records
    uint8_t* cfall;                      // [Cmax] placed at xhat
    int32_t* cnew;                       // [Cmax] index after compaction
    double* quad; double* xhat; double* pos;        // [Cmax][10], [Cmax][3], [Cmax][3]
    uint32_t* sblk; int64_t* soff;       // [nbS] heads per workgroup of sorted slots
    uint32_t* fblk; int64_t* foff;       // [nbF]
    uint32_t* cblk; int64_t* coff;       // [nbC]
};

// rule 2: floor((v - origin) * inv) saturated to [0, 2^21 - 1]; v is finite
__device__ __forceinline__ int64_t cell1(double v, double org, double inv) {
    double t = floor((v - org) * inv);
    t = t >= 0.0 ? t : 0.0;                                             // a NaN (0 * inf) goes to 0 too
    t = t <= 2097151.0 ? t : 2097151.0;
    return (int64_t)t;
}
__device__ __forceinline__ int64_t cell_key(const SimpArgs& a, int64_t v) {
    return (cell1(a.vert[3 * v], a.org[0], a.inv) << 42) | (cell1(a.vert[3 * v + 1], a.org[1], a.inv) << 21) |
           cell1(a.vert[3 * v + 2], a.org[2], a.inv);
}

// one thread per face: validity, the three corner keys, the face's edge uses
__global__ __launch_bounds__(WG) void simp_keys_kernel(SimpArgs a, int64_t* __restrict__ out_keys) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool invalid = false, repeated = false;
    if (f < a.F) {
        const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
        const bool ok = dudf_face_in_range(i0, i1, i2, a.V) && dudf_face_finite(a.vert, i0, i1, i2);
        invalid = !ok;
        repeated = ok && (i0 == i1 || i1 == i2 || i2 == i0);
        int64_t k0 = KEY_NONE, k1 = KEY_NONE, k2 = KEY_NONE;
        uint8_t f1 = 1, f2 = 2;
        if (ok && !repeated) {
            k0 = cell_key(a, i0); k1 = cell_key(a, i1); k2 = cell_key(a, i2);
            if (k1 == k0) { f1 = 0; k1 = KEY_NONE; }
            if (k2 == k0) { f2 = 0; k2 = KEY_NONE; } else if (f1 == 1 && k2 == k1) { f2 = 1; k2 = KEY_NONE; }
            const uint32_t idx[3] = {(uint32_t)i0, (uint32_t)i1, (uint32_t)i2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int64_t s = dudf_edge_claim(a.etab, a.capE, dudf_edge_key(idx[c], idx[c == 2 ? 0 : c + 1]));
                if (s >= 0) atomicAdd(&a.ecnt[s], 1u);
            }
        }
        a.fstate[f] = invalid ? ST_INVALID : repeated ? ST_REPEATED : ST_VALID;
        a.first[3 * f] = 0; a.first[3 * f + 1] = f1; a.first[3 * f + 2] = f2;
        out_keys[3 * f] = k0; out_keys[3 * f + 1] = k1; out_keys[3 * f + 2] = k2;
    }
    unsigned total;
    dudf_wg_rank(invalid, wt, &total);  dudf_wg_add_total(a.ctr + CTR_INVALID, total);
    dudf_wg_rank(repeated, wt, &total); dudf_wg_add_total(a.ctr + CTR_COLLAPSED, total);
}

// uses of the edge {u, w}, 0 when the table does not hold it (table complete: read only)
__device__ __forceinline__ uint32_t edge_uses(const SimpArgs& a, uint32_t u, uint32_t w) {
    const int64_t s = dudf_edge_slot(a.etab, a.capE, dudf_edge_key(u, w));
    return s >= 0 ? a.ecnt[s] : 0u;
}

// one thread per face: which of its edges exactly one valid face uses (each border edge belongs to one face: counted once)
__global__ __launch_bounds__(WG) void simp_border_kernel(SimpArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    unsigned m = 0;
    if (f < a.F && a.fstate[f] == ST_VALID) {
        const uint32_t i0 = (uint32_t)a.face[3 * f], i1 = (uint32_t)a.face[3 * f + 1], i2 = (uint32_t)a.face[3 * f + 2];
        m = (edge_uses(a, i0, i1) == 1u ? 1u : 0u) | (edge_uses(a, i1, i2) == 1u ? 2u : 0u) | (edge_uses(a, i2, i0) == 1u ? 4u : 0u);
    }
    if (f < a.F) a.fborder[f] = (uint8_t)m;
    unsigned total;
    dudf_wg_scan((unsigned)__popc(m), wt, &total);
    dudf_wg_add_total(a.ctr + CTR_BORDER, total);
}

// one thread per sorted slot.  PASS 0: heads of the runs per workgroup; PASS 1: the cell id of every record, the cell's start and key
template <int PASS>
__global__ __launch_bounds__(WG) void simp_heads_kernel(SimpArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t i = dudf_wg_item(), n = 3 * a.F;
    const int64_t key = i < n ? a.skey[i] : KEY_NONE;
    const bool rec = key >= 0;
    const bool hd = rec && (i == 0 || a.skey[i - 1] != key);
    unsigned total;
    const unsigned before = dudf_wg_rank(hd, wt, &total);
    if (PASS == 0) {
        if (threadIdx.x == 0) a.sblk[blockIdx.x] = total;
    } else if (rec) {
        const int64_t cid = a.soff[blockIdx.x] + before + (hd ? 1 : 0) - 1;
        const int64_t slot = a.perm[i];
        if (cid >= 0 && cid < a.Cmax && slot >= 0 && slot < n) {        // keys that are not this call's own sorted keys write nothing
            a.g[slot] = (int32_t)cid;
            if (hd) { a.cstart[cid] = (int32_t)i; a.ckey[cid] = key; }
        }
    }
}

// one thread per face: the cell ids of all three corners; fewer than three distinct cells collapse
__global__ __launch_bounds__(WG) void simp_remap_kernel(SimpArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool col = false;
    if (f < a.F && a.fstate[f] == ST_VALID) {
        const int32_t g0 = a.g[3 * f];
        const int32_t g1 = a.first[3 * f + 1] == 1 ? a.g[3 * f + 1] : g0;
        const int32_t g2 = a.first[3 * f + 2] == 2 ? a.g[3 * f + 2] : a.first[3 * f + 2] == 1 ? g1 : g0;
        a.g[3 * f + 1] = g1; a.g[3 * f + 2] = g2;
        col = g0 < 0 || g1 < 0 || g2 < 0 || g0 == g1 || g1 == g2 || g2 == g0;
        a.fstate[f] = col ? ST_COLLAPSED : ST_ALIVE;
    }
    unsigned total;
    dudf_wg_rank(col, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_COLLAPSED, total);
}

// the faces with three cells enter the face table (triples are read from `g`, which the launch before wrote)
__global__ __launch_bounds__(WG) void simp_face_insert_kernel(SimpArgs a) {
    const int64_t f = dudf_wg_item();
    if (f >= a.F || a.fstate[f] != ST_ALIVE) return;
    dudf_first_insert(a.ftab, a.capF, DudfTriItems{a.g}, f, a.F);
}

// a face survives when it is the smallest index of its cell set; survivors mark their cells
__global__ __launch_bounds__(WG) void simp_resolve_kernel(SimpArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool alive = false, dup = false;
    if (f < a.F && a.fstate[f] == ST_ALIVE) {
        const DudfTriItems items{a.g};
        const DudfTri k = items.key(f);
        const uint32_t firstf = dudf_first_find(a.ftab, a.capF, items, k, a.F);
        alive = firstf == (uint32_t)f || firstf == kTabEmpty32;          // a triple the table does not hold: the face stands for itself
        dup = !alive;
        if (!dup) { a.cuse[k.a] = 1; a.cuse[k.b] = 1; a.cuse[k.c] = 1; }
    }
    if (dup) a.fstate[f] = ST_DUPLICATE;                                // no probe reads another face's state
    unsigned total;
    dudf_wg_rank(dup, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_DUPLICATE, total);
    dudf_wg_rank(alive, wt, &total);
    if (threadIdx.x == 0) a.fblk[blockIdx.x] = total;
}

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// one border term of rule 5: the plane through the edge u -> w perpendicular to the face (normal n), weight wb / (e.e)
__device__ __forceinline__ void add_border(double (&q)[10], double wb, const double (&u)[3], const double (&w)[3], const double (&n)[3]) {
    const double e0 = w[0] - u[0], e1 = w[1] - u[1], e2 = w[2] - u[2];
    const double ee = dot3(e0, e1, e2, e0, e1, e2);
    if (!(ee > 0.0)) return;
    const double m0 = e1 * n[2] - e2 * n[1], m1 = e2 * n[0] - e0 * n[2], m2 = e0 * n[1] - e1 * n[0];
    const double dm = -dot3(m0, m1, m2, u[0], u[1], u[2]);
    q[0] += (wb * (m0 * m0)) / ee; q[1] += (wb * (m0 * m1)) / ee; q[2] += (wb * (m0 * m2)) / ee;
    q[3] += (wb * (m1 * m1)) / ee; q[4] += (wb * (m1 * m2)) / ee; q[5] += (wb * (m2 * m2)) / ee;
    q[6] += (wb * (dm * m0)) / ee; q[7] += (wb * (dm * m1)) / ee; q[8] += (wb * (dm * m2)) / ee;
    q[9] += (wb * (dm * dm)) / ee;
}

// one thread per occupied cell: walks the cell's run of records in order (rule 6), then places the representative (rule 7)
__global__ __launch_bounds__(WG) void simp_cells_kernel(SimpArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t c = dudf_wg_item(), n3 = 3 * a.F;
    bool fell = false;
    if (c < a.Cmax && c < a.tot[TOT_CELLS]) {
        const int64_t key = a.ckey[c];
        const double cc[3] = {(double)(key >> 42), (double)((key >> 21) & CELL_MASK), (double)(key & CELL_MASK)};
        const double oc[3] = {a.org[0] + (cc[0] + 0.5) * a.h, a.org[1] + (cc[1] + 0.5) * a.h, a.org[2] + (cc[2] + 0.5) * a.h};
        double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double xs0 = 0.0, xs1 = 0.0, xs2 = 0.0;
        int32_t count = 0;
        for (int64_t i = a.cstart[c]; i >= 0 && i < n3 && a.skey[i] == key; ++i) {
            const int64_t slot = a.perm[i];
            if (slot < 0 || slot >= n3) continue;
            const int64_t f = slot / 3;
            const int k0 = (int)(slot - 3 * f);
            if (a.fstate[f] < ST_VALID) continue;
            const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
            const double u0[3] = {(a.vert[3 * i0] - oc[0]) * a.inv, (a.vert[3 * i0 + 1] - oc[1]) * a.inv, (a.vert[3 * i0 + 2] - oc[2]) * a.inv};
            const double u1[3] = {(a.vert[3 * i1] - oc[0]) * a.inv, (a.vert[3 * i1 + 1] - oc[1]) * a.inv, (a.vert[3 * i1 + 2] - oc[2]) * a.inv};
            const double u2[3] = {(a.vert[3 * i2] - oc[0]) * a.inv, (a.vert[3 * i2 + 1] - oc[1]) * a.inv, (a.vert[3 * i2 + 2] - oc[2]) * a.inv};
            const double e0 = u1[0] - u0[0], e1 = u1[1] - u0[1], e2 = u1[2] - u0[2];
            const double g0 = u2[0] - u0[0], g1 = u2[1] - u0[1], g2 = u2[2] - u0[2];
            const double n[3] = {e1 * g2 - e2 * g1, e2 * g0 - e0 * g2, e0 * g1 - e1 * g0};
            const double d = -dot3(n[0], n[1], n[2], u0[0], u0[1], u0[2]);
            q[0] += n[0] * n[0]; q[1] += n[0] * n[1]; q[2] += n[0] * n[2]; q[3] += n[1] * n[1]; q[4] += n[1] * n[2]; q[5] += n[2] * n[2];
            q[6] += d * n[0]; q[7] += d * n[1]; q[8] += d * n[2]; q[9] += d * d;
            if (a.wb > 0.0) {
                const unsigned m = a.fborder[f];
                const bool in0 = a.g[3 * f] == (int32_t)c, in1 = a.g[3 * f + 1] == (int32_t)c, in2 = a.g[3 * f + 2] == (int32_t)c;
                if ((m & 1u) && (in0 || in1)) add_border(q, a.wb, u0, u1, n);
                if ((m & 2u) && (in1 || in2)) add_border(q, a.wb, u1, u2, n);
                if ((m & 4u) && (in2 || in0)) add_border(q, a.wb, u2, u0, n);
            }
            xs0 += k0 == 0 ? u0[0] : k0 == 1 ? u1[0] : u2[0];
            xs1 += k0 == 0 ? u0[1] : k0 == 1 ? u1[1] : u2[1];
            xs2 += k0 == 0 ? u0[2] : k0 == 1 ? u1[2] : u2[2];
            ++count;
        }
        const double cnt = (double)count;
        const double xh[3] = {xs0 / cnt, xs1 / cnt, xs2 / cnt};
        const double Hm[3][3] = {{q[0], 0.0, 0.0}, {q[1], q[3], 0.0}, {q[2], q[4], q[5]}};       // eigh3 reads the lower triangle
        double lam[3], E[3][3];
        eigh3(Hm, lam, E);
        const double l0 = fabs(lam[0]), l1 = fabs(lam[1]), l2 = fabs(lam[2]);
        const double lmax = fmax(fmax(l0, l1), l2);
        const bool bad = !(isfinite(lam[0]) && isfinite(lam[1]) && isfinite(lam[2])) || lmax == 0.0;
        const double r0 = -q[6] - dot3(q[0], q[1], q[2], xh[0], xh[1], xh[2]);
        const double r1 = -q[7] - dot3(q[1], q[3], q[4], xh[0], xh[1], xh[2]);
        const double r2 = -q[8] - dot3(q[2], q[4], q[5], xh[0], xh[1], xh[2]);
        double x0 = xh[0], x1 = xh[1], x2 = xh[2];
        if (!bad) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (lam[i] > a.tau * lmax) {
                    const double s = dot3(E[0][i], E[1][i], E[2][i], r0, r1, r2) / lam[i];
                    x0 += E[0][i] * s; x1 += E[1][i] * s; x2 += E[2][i] * s;
                }
        }
        fell = bad || !(fabs(x0) <= 0.5 && fabs(x1) <= 0.5 && fabs(x2) <= 0.5);
        if (fell) { x0 = xh[0]; x1 = xh[1]; x2 = xh[2]; }
#pragma unroll
        for (int j = 0; j < 10; ++j) a.quad[10 * c + j] = q[j];
        a.xhat[3 * c] = xh[0]; a.xhat[3 * c + 1] = xh[1]; a.xhat[3 * c + 2] = xh[2];
        a.pos[3 * c] = ((cc[0] + 0.5) + x0) * a.h + a.org[0];
        a.pos[3 * c + 1] = ((cc[1] + 0.5) + x1) * a.h + a.org[1];
        a.pos[3 * c + 2] = ((cc[2] + 0.5) + x2) * a.h + a.org[2];
        a.ccount[c] = count; a.cfall[c] = fell ? 1 : 0;
    }
    unsigned total;
    dudf_wg_rank(fell, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_FALLBACK, total);
}

__global__ __launch_bounds__(WG) void simp_used_kernel(SimpArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t c = dudf_wg_item();
    unsigned total;
    dudf_wg_rank(c < a.Cmax && a.cuse[c], wt, &total);
    if (threadIdx.x == 0) a.cblk[blockIdx.x] = total;
}

// out_counts: V', F', cells, collapsed, duplicate, invalid, border edges, fallback (-1: the cells were not placed)
__global__ void simp_finish_kernel(SimpArgs a, int placed, int64_t* out_counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out_counts[0] = a.tot[TOT_USED]; out_counts[1] = a.tot[TOT_FACES]; out_counts[2] = a.tot[TOT_CELLS];
    out_counts[3] = (int64_t)a.ctr[CTR_COLLAPSED]; out_counts[4] = (int64_t)a.ctr[CTR_DUPLICATE]; out_counts[5] = (int64_t)a.ctr[CTR_INVALID];
    out_counts[6] = (int64_t)a.ctr[CTR_BORDER]; out_counts[7] = placed ? (int64_t)a.ctr[CTR_FALLBACK] : -1;
    a.head[HEAD_MAGIC] = MAGIC_SIMPLIFY; a.head[HEAD_V] = a.V; a.head[HEAD_F] = a.F; a.head[HEAD_PLACED] = placed;
}

__device__ __forceinline__ bool head_ok(const SimpArgs& a) {
    return a.head[HEAD_MAGIC] == MAGIC_SIMPLIFY && a.head[HEAD_V] == a.V && a.head[HEAD_F] == a.F && a.head[HEAD_PLACED] == 1;
}

// one thread per cell: the used cells' positions in key order; with the optional outputs, every occupied cell's sums
__global__ __launch_bounds__(WG) void simp_emit_cells_kernel(SimpArgs a, double* __restrict__ out_v, double* __restrict__ out_quad,
                                                             double* __restrict__ out_xhat, int64_t* __restrict__ out_ckey,
                                                             int64_t* __restrict__ out_records, uint8_t* __restrict__ out_fell) {
    __shared__ unsigned wt[WG / 64];
    if (!head_ok(a)) return;                                            // uniform: the whole grid leaves
    const int64_t c = dudf_wg_item();
    const bool occ = c < a.Cmax && c < a.tot[TOT_CELLS];
    const bool use = occ && a.cuse[c];
    unsigned total;
    const unsigned r = dudf_wg_rank(use, wt, &total);
    if (use) {
        const int64_t n = a.coff[blockIdx.x] + r;
        a.cnew[c] = (int32_t)n;
        out_v[3 * n] = a.pos[3 * c]; out_v[3 * n + 1] = a.pos[3 * c + 1]; out_v[3 * n + 2] = a.pos[3 * c + 2];
    }
    if (occ && out_quad) {
#pragma unroll
        for (int j = 0; j < 10; ++j) out_quad[10 * c + j] = a.quad[10 * c + j];
        out_xhat[3 * c] = a.xhat[3 * c]; out_xhat[3 * c + 1] = a.xhat[3 * c + 1]; out_xhat[3 * c + 2] = a.xhat[3 * c + 2];
        out_ckey[c] = a.ckey[c]; out_records[c] = a.ccount[c]; out_fell[c] = a.cfall[c];
    }
}

__global__ __launch_bounds__(WG) void simp_emit_faces_kernel(SimpArgs a, int64_t* __restrict__ out_f) {
    __shared__ unsigned wt[WG / 64];
    if (!head_ok(a)) return;
    const int64_t f = dudf_wg_item();
    const bool alive = f < a.F && a.fstate[f] == ST_ALIVE;
    unsigned total;
    const unsigned r = dudf_wg_rank(alive, wt, &total);
    if (alive) {
        const int64_t n = a.foff[blockIdx.x] + r;
        out_f[3 * n] = a.cnew[a.g[3 * f]]; out_f[3 * n + 1] = a.cnew[a.g[3 * f + 1]]; out_f[3 * n + 2] = a.cnew[a.g[3 * f + 2]];
    }
}

// F == 0: a valid empty result
__global__ void simp_empty_kernel(int64_t* out_counts, int64_t* head) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < 8; ++i) out_counts[i] = 0;
    head[HEAD_MAGIC] = 0;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < (1ll << 31) && 3 * F < (1ll << 31); }

// zero-initialised arrays first, 0xff-initialised second, the rest behind (dudf_init_spans)
DudfSpans carve_simp(void* ws, int64_t V, int64_t F, SimpArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    a->V = V; a->F = F;
    a->capE = dudf_pow2_at_least(6 * F); a->capF = dudf_pow2_at_least(2 * F);
    a->Cmax = 3 * F < V ? 3 * F : V;                                    // every occupied cell holds a vertex and a record
    a->nbS = dudf_wg_count(3 * F); a->nbF = dudf_wg_count(F); a->nbC = dudf_wg_count(a->Cmax > 0 ? a->Cmax : 1);
    a->head = cv.take<int64_t>(N_HEAD); a->tot = cv.take<int64_t>(N_TOT); a->ctr = cv.take<unsigned long long>(N_CTR);
    a->ecnt = cv.take<uint32_t>(a->capE); a->cuse = cv.take<uint8_t>(a->Cmax);
    DudfSpans sp;
    sp.zero_end = sp.ff_begin = cv.o;
    a->etab = cv.take<unsigned long long>(a->capE); a->ftab = cv.take<uint32_t>(a->capF); a->g = cv.take<int32_t>(3 * F);
    a->cstart = cv.take<int32_t>(a->Cmax);
    sp.ff_end = cv.o;
    a->fstate = cv.take<uint8_t>(F); a->fborder = cv.take<uint8_t>(F); a->first = cv.take<uint8_t>(3 * F);
    a->ckey = cv.take<int64_t>(a->Cmax); a->ccount = cv.take<int32_t>(a->Cmax); a->cfall = cv.take<uint8_t>(a->Cmax);
    a->cnew = cv.take<int32_t>(a->Cmax);
    a->quad = cv.take<double>(10 * a->Cmax); a->xhat = cv.take<double>(3 * a->Cmax); a->pos = cv.take<double>(3 * a->Cmax);
    a->sblk = cv.take<uint32_t>(a->nbS); a->soff = cv.take<int64_t>(a->nbS);
    a->fblk = cv.take<uint32_t>(a->nbF); a->foff = cv.take<int64_t>(a->nbF);
    a->cblk = cv.take<uint32_t>(a->nbC); a->coff = cv.take<int64_t>(a->nbC);
    sp.total = cv.o;
    return sp;
}

// the checks of rule 10 that all three calls share, in front of any device call
int fill_simp(const double* vertices, int64_t V, const int64_t* faces, int64_t F, void* ws, size_t bytes, SimpArgs* a, DudfSpans* sp) {
    if (V < 0 || F < 0) return DUDF_E_BADCFG;
    if (!sizes_ok(V, F)) return DUDF_E_UNSUPPORTED;
    if (F > 0 && (!faces || (V > 0 && !vertices))) return DUDF_E_BADCFG;
    *sp = carve_simp(ws, V, F, a);
    if (int rc = dudf_check_buffer(ws, bytes, sp->total)) return rc;
    a->vert = vertices; a->face = faces; a->skey = nullptr; a->perm = nullptr;
    a->org[0] = a->org[1] = a->org[2] = 0.0; a->h = 1.0; a->inv = 1.0; a->wb = 0.0; a->tau = 1e-3;
    return 0;
}

bool cell_ok(const double* origin, double cell) {
    if (!origin || !(cell > 0.0) || !(cell <= 1.79769313486231570815e308)) return false;
    const double inv = 1.0 / cell;
    if (!(inv > 0.0) || !(inv <= 1.79769313486231570815e308)) return false;
    for (int d = 0; d < 3; ++d)
        if (!(origin[d] >= -1.79769313486231570815e308 && origin[d] <= 1.79769313486231570815e308)) return false;
    return true;
}

}  // namespace

extern "C" {

size_t dudf_mesh_simplify_workspace_bytes(int64_t V, int64_t F) {
    if (!sizes_ok(V, F)) return 0;
    SimpArgs a;
    return carve_simp(nullptr, V, F, &a).total;
}

int dudf_mesh_simplify_keys(const double* vertices, int64_t V, const int64_t* faces, int64_t F, const double* origin, double cell,
                            int64_t* out_keys, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cell_ok(origin, cell)) return DUDF_E_BADCFG;
    SimpArgs a; DudfSpans sp;
    int rc = fill_simp(vertices, V, faces, F, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (F > 0 && !out_keys) return DUDF_E_BADCFG;
    a.org[0] = origin[0]; a.org[1] = origin[1]; a.org[2] = origin[2]; a.h = cell; a.inv = 1.0 / cell;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    if (F == 0) return (int)hipMemsetAsync(workspace, 0, sp.zero_end, st);                  // head and counters: no faces
    DUDF_TRY(dudf_init_spans(workspace, sp, st));
    return dudf_launch(simp_keys_kernel, dim3((unsigned)a.nbF), dim3(WG), st, a, out_keys);
}

int dudf_mesh_simplify_count(const double* vertices, int64_t V, const int64_t* faces, int64_t F, const double* origin, double cell,
                             double boundary_weight, double tau, const int64_t* sorted_keys, const int64_t* order, int place,
                             int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cell_ok(origin, cell) || !(boundary_weight >= 0.0) || !(tau > 0.0 && tau < 1.0) || (place != 0 && place != 1)) return DUDF_E_BADCFG;
    SimpArgs a; DudfSpans sp;
    int rc = fill_simp(vertices, V, faces, F, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_counts || (F > 0 && (!sorted_keys || !order))) return DUDF_E_BADCFG;
    a.org[0] = origin[0]; a.org[1] = origin[1]; a.org[2] = origin[2]; a.h = cell; a.inv = 1.0 / cell;
    a.wb = boundary_weight <= 1.79769313486231570815e308 ? boundary_weight : 1.79769313486231570815e308; a.tau = tau;
    a.skey = sorted_keys; a.perm = order;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    if (F == 0) return dudf_launch(simp_empty_kernel, dim3(1), dim3(1), st, out_counts, a.head);
    const dim3 gs((unsigned)a.nbS), gf((unsigned)a.nbF), gc((unsigned)a.nbC), wg(WG);
    DUDF_TRY(dudf_launch(simp_border_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(simp_heads_kernel<0>, gs, wg, st, a));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, a.sblk, a.soff, a.nbS, a.tot + TOT_CELLS));
    DUDF_TRY(dudf_launch(simp_heads_kernel<1>, gs, wg, st, a));
    DUDF_TRY(dudf_launch(simp_remap_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(simp_face_insert_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(simp_resolve_kernel, gf, wg, st, a));
    if (place) DUDF_TRY(dudf_launch(simp_cells_kernel, gc, wg, st, a));
    DUDF_TRY(dudf_launch(simp_used_kernel, gc, wg, st, a));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, a.cblk, a.coff, a.nbC, a.tot + TOT_USED));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, a.fblk, a.foff, a.nbF, a.tot + TOT_FACES));
    return dudf_launch(simp_finish_kernel, dim3(1), dim3(1), st, a, place, out_counts);
}

int dudf_mesh_simplify_emit(const double* vertices, int64_t V, const int64_t* faces, int64_t F, double* out_vertices, int64_t* out_faces,
                            double* out_quadrics, double* out_xhat, int64_t* out_cell_keys, int64_t* out_records,
                            unsigned char* out_fallback, void* workspace, size_t workspace_bytes, void* stream) {
    SimpArgs a; DudfSpans sp;
    int rc = fill_simp(vertices, V, faces, F, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_vertices || !out_faces) return DUDF_E_BADCFG;
    if (out_quadrics && (!out_xhat || !out_cell_keys || !out_records || !out_fallback)) return DUDF_E_BADCFG;
    if (F == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    DUDF_TRY(dudf_launch(simp_emit_cells_kernel, dim3((unsigned)a.nbC), dim3(WG), st, a, out_vertices, out_quadrics, out_xhat, out_cell_keys,
                         out_records, (uint8_t*)out_fallback));
    return dudf_launch(simp_emit_faces_kernel, dim3((unsigned)a.nbF), dim3(WG), st, a, out_faces);
}

}  // extern "C"
