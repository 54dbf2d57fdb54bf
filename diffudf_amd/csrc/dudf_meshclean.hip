// Mesh clean-up behind `extract_mesh_MESHUDF` (reference src/render_mc.py:136-197) on the device: weld, prune, fill 3- and 4-edge
// holes, border edges, border smoothing.  The rules are DESIGN.md §3 "Mesh clean-up"; tests/meshclean_oracle.py restates them in
// numpy and the device result equals it bit for bit.  Built with -ffp-contract=off (the degenerate test and the smoothing repeat
// the oracle's double arithmetic).  Index work only: integer atomics on hash-table slots and counters, no float atomics.
//
// Hash tables, by the rules of dudf_meshtab.h:
//   vertices  smallest index per rounded position (VertItems below), capacity >= 2 V;
//   faces     smallest index per sorted remapped triple (read from `g`, which the launch before wrote), capacity >= 2 F;
//   edges     capacity >= 6 F; `einfo` beside a slot counts the uses (bits 0..30) and notes whether min -> max occurs as a directed
//             edge (bit 31).
#include "dudf_meshtab.h"

namespace {

constexpr int WG = DUDF_WG;
constexpr uint32_t DIR_BIT = 0x80000000u;
constexpr int64_t MAGIC_CLEAN = 0x6475646643314c4ell, MAGIC_BORDER = 0x6475646642314f52ll;
enum { ST_INVALID = 0, ST_DEGENERATE = 1, ST_DUPLICATE = 2, ST_ALIVE = 3 };
enum { CTR_INVALID = 0, CTR_REFERENCED, CTR_DISTINCT, CTR_DEGENERATE, CTR_DUPLICATE, N_CTR };
enum { TOT_KEEP = 0, TOT_H3, TOT_H4, TOT_ALIVE, N_TOT };

struct VKey { int64_t x, y, z; };
__device__ __forceinline__ int64_t key1(double c, double scale) {      // rint(c * 10^digits), saturated at the ends of int64
    double k = __builtin_rint(c * scale);
    k = fmin(fmax(k, -9223372036854775808.0), 9223372036854774784.0);
    return (int64_t)k;
}
struct VertItems {                                             // the vertices by their position rounded to `digits` decimals
    const double* vert; double scale;
    __device__ __forceinline__ VKey key(int64_t v) const {
        return VKey{key1(vert[3 * v], scale), key1(vert[3 * v + 1], scale), key1(vert[3 * v + 2], scale)};
    }
    __device__ __forceinline__ static bool same(const VKey& a, const VKey& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
    __device__ __forceinline__ static uint64_t hash(const VKey& k) {
        return dudf_mix64(dudf_mix64(dudf_mix64((uint64_t)k.x) ^ (uint64_t)k.y) ^ (uint64_t)k.z);
    }
};

// one use of the directed edge from -> to (from != to, both in [0, 2^31))
__device__ __forceinline__ void edge_insert(unsigned long long* __restrict__ etab, uint32_t* __restrict__ einfo, int64_t cap, int32_t from,
                                            int32_t to) {
    const int64_t s = dudf_edge_claim(etab, cap, dudf_edge_key((uint32_t)from, (uint32_t)to));
    if (s < 0) return;
    atomicAdd(&einfo[s], 1u);
    if (from < to) atomicOr(&einfo[s], DIR_BIT);
}

// ---------------------------------------------------------------------------------------------------------------- clean-up round
struct CleanArgs {
    const double* vert; const int64_t* face; int64_t V, F; double scale; int fill;
    int64_t capV, capF, capE, nbV, nbF;
    int64_t* head;                       // [4] magic, V, F, fill: what the workspace holds (emit checks it on the device)
    int64_t* tot;                        // [N_TOT] scan totals: kept vertices, 3-holes, 4-holes, surviving faces
    unsigned long long* ctr;             // [N_CTR]
    int32_t* rep;                        // [V] representative, -1: no valid face uses the vertex
    int32_t* vnew;                       // [V] index after compaction
    int32_t* bdeg; int32_t* bnb;         // [V], [V][2] border degree and the first two border neighbours
    uint8_t* vref; uint8_t* vkeep; uint8_t* hole;   // [V] used by a valid / a surviving face; 1 = closes a 3-hole, 2 = a 4-hole
    uint32_t* vtab;                      // [capV]
    int32_t* g;                          // [F][3] faces over representatives
    uint8_t* fstate;                     // [F] ST_*
    uint32_t* ftab;                      // [capF]
    unsigned long long* etab; uint32_t* einfo;      // [capE]
    uint32_t* vblk; int64_t* voff;       // [nbV][3]
    uint32_t* fblk; int64_t* foff;       // [nbF]
    double* out_v; int64_t* out_f;
};

__global__ __launch_bounds__(WG) void clean_validate_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool bad = false;
    if (f < a.F) {
        const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
        const bool ok = dudf_face_in_range(i0, i1, i2, a.V) && dudf_face_finite(a.vert, i0, i1, i2);
        a.fstate[f] = ok ? ST_ALIVE : ST_INVALID;
        if (ok) { a.vref[i0] = 1; a.vref[i1] = 1; a.vref[i2] = 1; }
        bad = !ok;
    }
    unsigned total;
    dudf_wg_rank(bad, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_INVALID, total);
}

__global__ __launch_bounds__(WG) void clean_weld_insert_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t v = dudf_wg_item();
    const bool ref = v < a.V && a.vref[v];
    const bool claimed = ref && dudf_first_insert(a.vtab, a.capV, VertItems{a.vert, a.scale}, v, a.V);
    unsigned total;
    dudf_wg_rank(ref, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_REFERENCED, total);
    dudf_wg_rank(claimed, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_DISTINCT, total);
}

__global__ __launch_bounds__(WG) void clean_weld_resolve_kernel(CleanArgs a) {
    const int64_t v = dudf_wg_item();
    if (v >= a.V) return;
    const VertItems items{a.vert, a.scale};
    a.rep[v] = a.vref[v] ? (int32_t)dudf_first_find(a.vtab, a.capV, items, items.key(v), a.V) : -1;      // absent: kTabEmpty32 is -1 too
}

__device__ __forceinline__ double sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }

__global__ __launch_bounds__(WG) void clean_remap_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool deg = false;
    if (f < a.F && a.fstate[f] == ST_ALIVE) {
        const int32_t g0 = a.rep[a.face[3 * f]], g1 = a.rep[a.face[3 * f + 1]], g2 = a.rep[a.face[3 * f + 2]];
        a.g[3 * f] = g0; a.g[3 * f + 1] = g1; a.g[3 * f + 2] = g2;
        const double* p0 = a.vert + 3 * (int64_t)g0; const double* p1 = a.vert + 3 * (int64_t)g1; const double* p2 = a.vert + 3 * (int64_t)g2;
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double ex = p2[0] - p1[0], ey = p2[1] - p1[1], ez = p2[2] - p1[2];
        const double l2 = fmax(fmax(sq3(ax, ay, az), sq3(ex, ey, ez)), sq3(bx, by, bz));
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        deg = (l2 <= 1e-16) || (sq3(cx, cy, cz) <= 1e-16 * l2);
        if (deg) a.fstate[f] = ST_DEGENERATE;
    }
    unsigned total;
    dudf_wg_rank(deg, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_DEGENERATE, total);
}

__global__ __launch_bounds__(WG) void clean_face_insert_kernel(CleanArgs a) {
    const int64_t f = dudf_wg_item();
    if (f >= a.F || a.fstate[f] != ST_ALIVE) return;
    dudf_first_insert(a.ftab, a.capF, DudfTriItems{a.g}, f, a.F);
}

// a face survives when it is the smallest index of its vertex set; survivors mark their vertices and enter their edges
__global__ __launch_bounds__(WG) void clean_face_resolve_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool alive = false, dup = false;
    if (f < a.F && a.fstate[f] == ST_ALIVE) {
        const DudfTriItems items{a.g};
        const uint32_t first = dudf_first_find(a.ftab, a.capF, items, items.key(f), a.F);
        alive = first == (uint32_t)f || first == kTabEmpty32;            // a triple the table does not hold: the face stands for itself
        dup = !alive;
        if (dup) a.fstate[f] = ST_DUPLICATE;
        else {
            const int32_t g0 = a.g[3 * f], g1 = a.g[3 * f + 1], g2 = a.g[3 * f + 2];
            a.vkeep[g0] = 1; a.vkeep[g1] = 1; a.vkeep[g2] = 1;
            if (a.fill) {
                edge_insert(a.etab, a.einfo, a.capE, g0, g1);
                edge_insert(a.etab, a.einfo, a.capE, g1, g2);
                edge_insert(a.etab, a.einfo, a.capE, g2, g0);
            }
        }
    }
    unsigned total;
    dudf_wg_rank(dup, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_DUPLICATE, total);
    dudf_wg_rank(alive, wt, &total);
    if (threadIdx.x == 0) a.fblk[blockIdx.x] = total;
}

// border edges (one use) -> degree and the first two neighbours of their endpoints
__global__ __launch_bounds__(WG) void clean_border_adj_kernel(CleanArgs a) {
    const int64_t s = dudf_wg_item();
    if (s >= a.capE) return;
    const unsigned long long key = a.etab[s];
    if (key == kTabEmpty64 || (a.einfo[s] & ~DIR_BIT) != 1u) return;
    const int32_t u = (int32_t)(key >> 32), w = (int32_t)(key & 0xffffffffu);
    int i = atomicAdd(&a.bdeg[u], 1);
    if (i < 2) a.bnb[2 * (int64_t)u + i] = w;
    i = atomicAdd(&a.bdeg[w], 1);
    if (i < 2) a.bnb[2 * (int64_t)w + i] = u;
}

// The border cycle through `va` when it is a whole hole of 3 or 4 vertices of border degree 2 whose smallest vertex is `va`:
// returns its length (0: none), b < d the neighbours of a, c the vertex opposite a (4-cycles).  At most four steps.
__device__ __forceinline__ int hole_walk(const CleanArgs& a, int32_t va, int32_t* b, int32_t* c, int32_t* d) {
    const int32_t n0 = a.bnb[2 * (int64_t)va], n1 = a.bnb[2 * (int64_t)va + 1];
    *b = n0 < n1 ? n0 : n1; *d = n0 < n1 ? n1 : n0; *c = -1;
    int32_t prev = va, cur = *b;
    int len = 1;
    for (int step = 0; step < 4; ++step) {
        if (cur == va) return len >= 3 ? len : 0;
        if (len == 4 || cur < va || a.bdeg[cur] != 2) return 0;
        if (len == 2) *c = cur;
        const int32_t m0 = a.bnb[2 * (int64_t)cur], m1 = a.bnb[2 * (int64_t)cur + 1];
        const int32_t next = m0 == prev ? m1 : m0;
        prev = cur; cur = next; ++len;
    }
    return 0;
}

__global__ __launch_bounds__(WG) void clean_holes_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t v = dudf_wg_item();
    const bool keep = v < a.V && a.vkeep[v];
    int h = 0;
    if (keep && a.fill && a.bdeg[v] == 2) {
        int32_t b, c, d;
        const int len = hole_walk(a, (int32_t)v, &b, &c, &d);
        h = len == 3 ? 1 : len == 4 ? 2 : 0;
    }
    if (v < a.V) a.hole[v] = (uint8_t)h;
    unsigned t0, t1, t2;
    dudf_wg_rank(keep, wt, &t0);
    dudf_wg_rank(h == 1, wt, &t1);
    dudf_wg_rank(h == 2, wt, &t2);
    if (threadIdx.x == 0) { a.vblk[3 * (int64_t)blockIdx.x] = t0; a.vblk[3 * (int64_t)blockIdx.x + 1] = t1; a.vblk[3 * (int64_t)blockIdx.x + 2] = t2; }
}

// out_counts: V', F', welded, unreferenced, duplicate faces, degenerate faces, 3-holes, 4-holes, invalid faces
__global__ void clean_finish_kernel(CleanArgs a, int64_t* out_counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t welded = (int64_t)a.ctr[CTR_REFERENCED] - (int64_t)a.ctr[CTR_DISTINCT];
    out_counts[0] = a.tot[TOT_KEEP];
    out_counts[1] = a.tot[TOT_ALIVE] + a.tot[TOT_H3] + 2 * a.tot[TOT_H4];
    out_counts[2] = welded;
    out_counts[3] = a.V - welded - a.tot[TOT_KEEP];
    out_counts[4] = (int64_t)a.ctr[CTR_DUPLICATE];
    out_counts[5] = (int64_t)a.ctr[CTR_DEGENERATE];
    out_counts[6] = a.tot[TOT_H3];
    out_counts[7] = a.tot[TOT_H4];
    out_counts[8] = (int64_t)a.ctr[CTR_INVALID];
    a.head[0] = MAGIC_CLEAN; a.head[1] = a.V; a.head[2] = a.F; a.head[3] = a.fill;
}

// V == 0 or F == 0: nothing survives
__global__ void clean_empty_kernel(int64_t V, int64_t F, int64_t* out_counts, int64_t* head) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < 9; ++i) out_counts[i] = 0;
    out_counts[3] = V; out_counts[8] = F;
    head[0] = 0;
}

__device__ __forceinline__ bool clean_head_ok(const CleanArgs& a) {
    return a.head[0] == MAGIC_CLEAN && a.head[1] == a.V && a.head[2] == a.F && a.head[3] == a.fill;
}

__global__ __launch_bounds__(WG) void clean_emit_vertices_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    if (!clean_head_ok(a)) return;                                      // uniform: the whole grid leaves
    const int64_t v = dudf_wg_item();
    const bool keep = v < a.V && a.vkeep[v];
    unsigned total;
    const unsigned r = dudf_wg_rank(keep, wt, &total);
    if (keep) {
        const int64_t n = a.voff[3 * (int64_t)blockIdx.x] + r;
        a.vnew[v] = (int32_t)n;
        a.out_v[3 * n] = a.vert[3 * v]; a.out_v[3 * n + 1] = a.vert[3 * v + 1]; a.out_v[3 * n + 2] = a.vert[3 * v + 2];
    }
}

__global__ __launch_bounds__(WG) void clean_emit_faces_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    if (!clean_head_ok(a)) return;
    const int64_t f = dudf_wg_item();
    const bool alive = f < a.F && a.fstate[f] == ST_ALIVE;
    unsigned total;
    const unsigned r = dudf_wg_rank(alive, wt, &total);
    if (alive) {
        const int64_t n = a.foff[blockIdx.x] + r;
        a.out_f[3 * n] = a.vnew[a.g[3 * f]]; a.out_f[3 * n + 1] = a.vnew[a.g[3 * f + 1]]; a.out_f[3 * n + 2] = a.vnew[a.g[3 * f + 2]];
    }
}

// the faces that close the holes, behind the surviving faces, holes in ascending smallest vertex
__global__ __launch_bounds__(WG) void clean_emit_holes_kernel(CleanArgs a) {
    __shared__ unsigned wt[WG / 64];
    if (!clean_head_ok(a)) return;
    const int64_t v = dudf_wg_item();
    const unsigned h = v < a.V ? a.hole[v] : 0;
    unsigned total;
    const unsigned before = dudf_wg_scan(h, wt, &total);
    if (!h) return;
    int32_t b, c, d;
    if (hole_walk(a, (int32_t)v, &b, &c, &d) != (int)h + 2) return;
    const int64_t s = dudf_edge_slot(a.etab, a.capE, dudf_edge_key((uint32_t)v, (uint32_t)b));
    const bool rev = s >= 0 && (a.einfo[s] & DIR_BIT) != 0;            // a face already runs a -> b
    const int64_t n = a.tot[TOT_ALIVE] + a.voff[3 * (int64_t)blockIdx.x + 1] + 2 * a.voff[3 * (int64_t)blockIdx.x + 2] + before;
    const int64_t na = a.vnew[v], nb = a.vnew[b], nd = a.vnew[d];
    int64_t* o = a.out_f + 3 * n;
    if (h == 1) {
        o[0] = rev ? nd : na; o[1] = nb; o[2] = rev ? na : nd;
    } else {
        const int64_t nc = a.vnew[c];
        o[0] = rev ? nc : na; o[1] = nb; o[2] = rev ? na : nc;
        o[3] = rev ? na : nc; o[4] = nd; o[5] = rev ? nc : na;
    }
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < (1ll << 31) && F < (1ll << 31); }

// zero-initialised arrays first, 0xff-initialised tables second, the rest behind (dudf_init_spans)
DudfSpans carve_clean(void* ws, int64_t V, int64_t F, CleanArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    a->V = V; a->F = F;
    a->capV = dudf_pow2_at_least(2 * V); a->capF = dudf_pow2_at_least(2 * F); a->capE = dudf_pow2_at_least(6 * F);
    a->nbV = dudf_wg_count(V); a->nbF = dudf_wg_count(F);
    a->head = cv.take<int64_t>(4); a->tot = cv.take<int64_t>(N_TOT); a->ctr = cv.take<unsigned long long>(N_CTR);
    a->vref = cv.take<uint8_t>(V); a->vkeep = cv.take<uint8_t>(V); a->hole = cv.take<uint8_t>(V);
    a->bdeg = cv.take<int32_t>(V); a->einfo = cv.take<uint32_t>(a->capE);
    DudfSpans sp;
    sp.zero_end = sp.ff_begin = cv.o;
    a->vtab = cv.take<uint32_t>(a->capV); a->ftab = cv.take<uint32_t>(a->capF); a->etab = cv.take<unsigned long long>(a->capE);
    sp.ff_end = cv.o;
    a->rep = cv.take<int32_t>(V); a->vnew = cv.take<int32_t>(V); a->bnb = cv.take<int32_t>(2 * V);
    a->g = cv.take<int32_t>(3 * F); a->fstate = cv.take<uint8_t>(F);
    a->vblk = cv.take<uint32_t>(3 * a->nbV); a->voff = cv.take<int64_t>(3 * a->nbV);
    a->fblk = cv.take<uint32_t>(a->nbF); a->foff = cv.take<int64_t>(a->nbF);
    sp.total = cv.o;
    return sp;
}

const double kPow10[16] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

int fill_clean(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int digits, int fill, void* ws, size_t bytes,
               CleanArgs* a, DudfSpans* sp) {
    if (V < 0 || F < 0 || digits < 0 || digits > 15 || (fill != 0 && fill != 1)) return DUDF_E_BADCFG;
    if (!sizes_ok(V, F)) return DUDF_E_UNSUPPORTED;
    if ((V > 0 && !vertices) || (F > 0 && !faces)) return DUDF_E_BADCFG;
    *sp = carve_clean(ws, V, F, a);
    if (int rc = dudf_check_buffer(ws, bytes, sp->total)) return rc;
    a->vert = vertices; a->face = faces; a->scale = kPow10[digits]; a->fill = fill;
    a->out_v = nullptr; a->out_f = nullptr;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ border edges, smoothing
struct BorderArgs {
    const int64_t* face; int64_t V, F, capE, nbV;
    int64_t* head;                       // [3] magic, V, F
    int64_t* tot;                        // [2] neighbour entries (2 E), border edges E
    int32_t* deg; int32_t* up; int32_t* cur;        // [V] border degree, neighbours above the vertex, fill cursor
    uint32_t* einfo; unsigned long long* etab;      // [capE]
    int64_t* coff; int64_t* uoff;        // [V] start of the vertex in nbr / in the edge list
    int32_t* nbr;                        // [6 F] border neighbours per vertex, ascending
    uint32_t* blk; int64_t* off;         // [nbV][2]
    double* pos;                         // [V][3] the second position buffer of the smoothing
};

__global__ __launch_bounds__(WG) void border_faces_kernel(BorderArgs a) {
    const int64_t f = dudf_wg_item();
    if (f >= a.F) return;
    const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
    if (!dudf_face_in_range(i0, i1, i2, a.V)) return;                   // skipped, never dereferenced
    const int32_t g0 = (int32_t)i0, g1 = (int32_t)i1, g2 = (int32_t)i2;
    if (g0 != g1) edge_insert(a.etab, a.einfo, a.capE, g0, g1);
    if (g1 != g2) edge_insert(a.etab, a.einfo, a.capE, g1, g2);
    if (g2 != g0) edge_insert(a.etab, a.einfo, a.capE, g2, g0);
}

template <int FILL>
__global__ __launch_bounds__(WG) void border_slots_kernel(BorderArgs a) {
    const int64_t s = dudf_wg_item();
    if (s >= a.capE) return;
    const unsigned long long key = a.etab[s];
    if (key == kTabEmpty64 || (a.einfo[s] & ~DIR_BIT) != 1u) return;
    const int32_t u = (int32_t)(key >> 32), w = (int32_t)(key & 0xffffffffu);
    if (!FILL) {
        atomicAdd(&a.deg[u], 1); atomicAdd(&a.deg[w], 1); atomicAdd(&a.up[u], 1);
    } else {                                                             // arrival order: border_sort_kernel orders the lists
        a.nbr[a.coff[u] + atomicAdd(&a.cur[u], 1)] = w;
        a.nbr[a.coff[w] + atomicAdd(&a.cur[w], 1)] = u;
    }
}

template <int PASS>
__global__ __launch_bounds__(WG) void border_offsets_kernel(BorderArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t v = dudf_wg_item();
    const unsigned d = v < a.V ? (unsigned)a.deg[v] : 0u, u = v < a.V ? (unsigned)a.up[v] : 0u;
    unsigned t0, t1;
    const unsigned b0 = dudf_wg_scan(d, wt, &t0);
    const unsigned b1 = dudf_wg_scan(u, wt, &t1);
    if (PASS == 0) {
        if (threadIdx.x == 0) { a.blk[2 * (int64_t)blockIdx.x] = t0; a.blk[2 * (int64_t)blockIdx.x + 1] = t1; }
    } else if (v < a.V) {
        a.coff[v] = a.off[2 * (int64_t)blockIdx.x] + b0;
        a.uoff[v] = a.off[2 * (int64_t)blockIdx.x + 1] + b1;
    }
}

__global__ __launch_bounds__(WG) void border_sort_kernel(BorderArgs a) {
    const int64_t v = dudf_wg_item();
    if (v == 0) { a.head[0] = MAGIC_BORDER; a.head[1] = a.V; a.head[2] = a.F; }
    if (v >= a.V) return;
    int32_t* l = a.nbr + a.coff[v];
    const int n = a.deg[v];
    for (int i = 1; i < n; ++i) {                                       // short lists: insertion sort in place
        const int32_t x = l[i];
        int j = i - 1;
        for (; j >= 0 && l[j] > x; --j) l[j + 1] = l[j];
        l[j + 1] = x;
    }
}

__device__ __forceinline__ bool border_head_ok(const BorderArgs& a) { return a.head[0] == MAGIC_BORDER && a.head[1] == a.V && a.head[2] == a.F; }

__global__ void border_count_kernel(BorderArgs a, int64_t* out_count) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out_count[0] = a.tot[1];
}

__global__ __launch_bounds__(WG) void border_emit_kernel(BorderArgs a, int64_t* __restrict__ out_edges) {
    if (!border_head_ok(a)) return;
    const int64_t v = dudf_wg_item();
    if (v >= a.V) return;
    const int32_t* l = a.nbr + a.coff[v];
    const int n = a.deg[v];
    int64_t o = a.uoff[v];
    for (int i = 0; i < n; ++i)
        if (l[i] > v) { out_edges[2 * o] = v; out_edges[2 * o + 1] = l[i]; ++o; }
}

// one Jacobi iteration src -> dst: border vertices move towards the mean of their border neighbours, the others are copied
__global__ __launch_bounds__(WG) void border_smooth_kernel(BorderArgs a, const double* __restrict__ src, double* __restrict__ dst, double lam) {
    if (!border_head_ok(a)) return;
    const int64_t v = dudf_wg_item();
    if (v >= a.V) return;
    const double x = src[3 * v], y = src[3 * v + 1], z = src[3 * v + 2];
    const int n = a.deg[v];
    if (n == 0) { dst[3 * v] = x; dst[3 * v + 1] = y; dst[3 * v + 2] = z; return; }
    const int32_t* l = a.nbr + a.coff[v];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = 0; i < n; ++i) { const int64_t w = l[i]; sx += src[3 * w]; sy += src[3 * w + 1]; sz += src[3 * w + 2]; }
    const double dn = (double)n;
    dst[3 * v] = x + lam * (sx / dn - x); dst[3 * v + 1] = y + lam * (sy / dn - y); dst[3 * v + 2] = z + lam * (sz / dn - z);
}

DudfSpans carve_border(void* ws, int64_t V, int64_t F, BorderArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    a->V = V; a->F = F; a->capE = dudf_pow2_at_least(6 * F); a->nbV = dudf_wg_count(V);
    a->head = cv.take<int64_t>(3); a->tot = cv.take<int64_t>(2);
    a->deg = cv.take<int32_t>(V); a->up = cv.take<int32_t>(V); a->cur = cv.take<int32_t>(V); a->einfo = cv.take<uint32_t>(a->capE);
    DudfSpans sp;
    sp.zero_end = sp.ff_begin = cv.o;
    a->etab = cv.take<unsigned long long>(a->capE);
    sp.ff_end = cv.o;
    a->coff = cv.take<int64_t>(V); a->uoff = cv.take<int64_t>(V); a->nbr = cv.take<int32_t>(6 * F);
    a->blk = cv.take<uint32_t>(2 * a->nbV); a->off = cv.take<int64_t>(2 * a->nbV);
    a->pos = cv.take<double>(3 * V);
    sp.total = cv.o;
    return sp;
}

bool border_sizes_ok(int64_t V, int64_t F) { return sizes_ok(V, F) && 6 * F < (1ll << 32); }   // block sums of degrees are 32-bit

int fill_border(int64_t V, const int64_t* faces, int64_t F, void* ws, size_t bytes, BorderArgs* a, DudfSpans* sp) {
    if (V < 0 || F < 0) return DUDF_E_BADCFG;
    if (!border_sizes_ok(V, F)) return DUDF_E_UNSUPPORTED;
    if (F > 0 && !faces) return DUDF_E_BADCFG;
    *sp = carve_border(ws, V, F, a);
    if (int rc = dudf_check_buffer(ws, bytes, sp->total)) return rc;
    a->face = faces;
    return 0;
}

// edge table -> per-vertex ascending lists of border neighbours (and the totals); V, F >= 1
int build_border(const BorderArgs& a, const DudfSpans& sp, void* ws, hipStream_t st) {
    DUDF_TRY(dudf_init_spans(ws, sp, st));
    const dim3 gv((unsigned)a.nbV), gf((unsigned)dudf_wg_count(a.F)), gs((unsigned)dudf_wg_count(a.capE)), wg(WG);
    DUDF_TRY(dudf_launch(border_faces_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(border_slots_kernel<0>, gs, wg, st, a));
    DUDF_TRY(dudf_launch(border_offsets_kernel<0>, gv, wg, st, a));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<2>, dim3(1), dim3(1024), st, a.blk, a.off, a.nbV, a.tot));
    DUDF_TRY(dudf_launch(border_offsets_kernel<1>, gv, wg, st, a));
    DUDF_TRY(dudf_launch(border_slots_kernel<1>, gs, wg, st, a));
    return dudf_launch(border_sort_kernel, gv, wg, st, a);
}

}  // namespace

extern "C" {

size_t dudf_mesh_clean_workspace_bytes(int64_t V, int64_t F) {
    if (!sizes_ok(V, F)) return 0;
    CleanArgs a;
    return carve_clean(nullptr, V, F, &a).total;
}

int dudf_mesh_clean_count(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int digits, int fill_holes,
                          int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
    CleanArgs a; DudfSpans sp;
    int rc = fill_clean(vertices, V, faces, F, digits, fill_holes, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_counts) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    if (V == 0 || F == 0) return dudf_launch(clean_empty_kernel, dim3(1), dim3(1), st, V, F, out_counts, a.head);
    DUDF_TRY(dudf_init_spans(workspace, sp, st));
    const dim3 gv((unsigned)a.nbV), gf((unsigned)a.nbF), wg(WG);
    DUDF_TRY(dudf_launch(clean_validate_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(clean_weld_insert_kernel, gv, wg, st, a));
    DUDF_TRY(dudf_launch(clean_weld_resolve_kernel, gv, wg, st, a));
    DUDF_TRY(dudf_launch(clean_remap_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(clean_face_insert_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(clean_face_resolve_kernel, gf, wg, st, a));
    if (a.fill) DUDF_TRY(dudf_launch(clean_border_adj_kernel, dim3((unsigned)dudf_wg_count(a.capE)), wg, st, a));
    DUDF_TRY(dudf_launch(clean_holes_kernel, gv, wg, st, a));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<3>, dim3(1), dim3(1024), st, a.vblk, a.voff, a.nbV, a.tot));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, a.fblk, a.foff, a.nbF, a.tot + TOT_ALIVE));
    return dudf_launch(clean_finish_kernel, dim3(1), dim3(1), st, a, out_counts);
}

int dudf_mesh_clean_emit(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int digits, int fill_holes,
                         double* out_vertices, int64_t* out_faces, void* workspace, size_t workspace_bytes, void* stream) {
    CleanArgs a; DudfSpans sp;
    int rc = fill_clean(vertices, V, faces, F, digits, fill_holes, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_vertices || !out_faces) return DUDF_E_BADCFG;
    if (V == 0 || F == 0) return 0;
    a.out_v = out_vertices; a.out_f = out_faces;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const dim3 gv((unsigned)a.nbV), gf((unsigned)a.nbF), wg(WG);
    DUDF_TRY(dudf_launch(clean_emit_vertices_kernel, gv, wg, st, a));
    DUDF_TRY(dudf_launch(clean_emit_faces_kernel, gf, wg, st, a));
    if (a.fill) DUDF_TRY(dudf_launch(clean_emit_holes_kernel, gv, wg, st, a));
    return 0;
}

size_t dudf_mesh_border_workspace_bytes(int64_t V, int64_t F) {
    if (!border_sizes_ok(V, F)) return 0;
    BorderArgs a;
    return carve_border(nullptr, V, F, &a).total;
}

int dudf_mesh_border_count(int64_t V, const int64_t* faces, int64_t F, int64_t* out_count, void* workspace, size_t workspace_bytes,
                           void* stream) {
    BorderArgs a; DudfSpans sp;
    int rc = fill_border(V, faces, F, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_count) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    if (V == 0 || F == 0) {
        DUDF_TRY(hipMemsetAsync(workspace, 0, sp.zero_end, st));        // head and totals: no edges
        return (int)hipMemsetAsync(out_count, 0, sizeof(int64_t), st);
    }
    rc = build_border(a, sp, workspace, st);
    if (rc) return rc;
    return dudf_launch(border_count_kernel, dim3(1), dim3(1), st, a, out_count);
}

int dudf_mesh_border_edges(int64_t V, const int64_t* faces, int64_t F, int64_t* out_edges, void* workspace, size_t workspace_bytes,
                           void* stream) {
    BorderArgs a; DudfSpans sp;
    int rc = fill_border(V, faces, F, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_edges) return DUDF_E_BADCFG;
    if (V == 0 || F == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(border_emit_kernel, dim3((unsigned)a.nbV), dim3(WG), st, a, out_edges);
}

int dudf_mesh_smooth_borders(double* vertices_inout, int64_t V, const int64_t* faces, int64_t F, int iterations, double lambda,
                             void* workspace, size_t workspace_bytes, void* stream) {
    BorderArgs a; DudfSpans sp;
    int rc = fill_border(V, faces, F, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (iterations < 0 || (V > 0 && !vertices_inout)) return DUDF_E_BADCFG;
    if (V == 0 || F == 0 || iterations == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    rc = build_border(a, sp, workspace, st);
    if (rc) return rc;
    double* src = vertices_inout; double* dst = a.pos;
    for (int it = 0; it < iterations; ++it) {                           // ping-pong: every average reads the positions before the iteration
        DUDF_TRY(dudf_launch(border_smooth_kernel, dim3((unsigned)a.nbV), dim3(WG), st, a, (const double*)src, dst, lambda));
        double* t = src; src = dst; dst = t;
    }
    if (src != vertices_inout)
        DUDF_TRY(hipMemcpyAsync(vertices_inout, src, (size_t)V * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // extern "C"
