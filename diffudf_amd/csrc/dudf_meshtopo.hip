// Mesh topology on the device: consistent winding, connected components with their face counts and integer areas, and the submesh of
// a face mask — what the reference's users ask of trimesh's `fix_winding` / `split` once a CAP-UDF soup has been welded.  The rules
// are DESIGN.md §3.6b; tests/meshtopo_oracle.py restates them in numpy and the device result equals it exactly.  Built with
// -ffp-contract=off (the face-normal length repeats the oracle's double arithmetic).  Index work only: integer atomics on hash-table
// slots, union-find words and counters, no float atomics.
//
// Edge table (dudf_meshtab.h, capacity >= 6 F): beside a slot the use count and the atomicMin / atomicMax of the face-slot ids
// e = 3 f + c that use it — the two faces of a manifold edge, whatever the arrival order.  Directions are re-read from the immutable
// faces.  A resolve pass turns the table into link[e]: the partner face-slot of e and the relative sign, or NONE; the rounds below
// never probe for their own edges again.
//
// Forest.  Borůvka over the links with a union-find whose word per face is (parent << 1) | parity to parent, as DESIGN.md §3.7: a
// round takes the minimum key of every component by 64-bit atomicMin, hooks along it (a mutual pair keeps the smaller
// representative) and flattens (parent, parity) by pointer doubling between two buffers.  Keys are distinct per link, so hooks form
// no cycle but the mutual pair.  Every loop has a trip count known at launch: probe loops are bounded by the capacity, rounds by
// ceil(log2 F) + 1, doubling steps by ceil(log2 F).
#include "dudf_meshtab.h"

namespace {

constexpr int WG = DUDF_WG;
constexpr uint32_t NONE32 = 0xffffffffu;
constexpr uint32_t SAME_BIT = 0x80000000u;
constexpr int64_t MAGIC_SUBMESH = 0x6475646653314d42ll;
enum { CTR_COMPONENTS = 0, CTR_FOREST, CTR_MANIFOLD,            // the order of out_counts
 CTR_BORDER, CTR_NONMANIFOLD, CTR_IGNORED, CTR_FLIPPED, CTR_INCONSISTENT, N_CTR };

struct TopoArgs {
    const int64_t* face; const double* vert; int64_t F, V, cap;
    unsigned long long* ctr;             // [N_CTR]
    unsigned* flags;                     // [64] a doubling step moved something
    uint32_t* ecnt; uint32_t* emax;      // [cap] uses, largest face-slot id
    unsigned long long* etab;            // [cap] keys
    uint32_t* emin;                      // [cap] smallest face-slot id
    uint32_t* label;                     // [F] per representative: the smallest face index of its component
    uint32_t* pp[2];                     // [F] each: the union-find words, ping-pong
    unsigned long long* best;            // [F] the best key of a round
    uint32_t* link;                      // [3 F] partner face-slot | SAME_BIT, or NONE32
    uint8_t* valid;                      // [F]
};

// the directed edge of face-slot e = 3 f + c of a valid face: indices c and (c + 1) % 3
__device__ __forceinline__ void slot_edge(const int64_t* __restrict__ face, uint32_t e, uint32_t* from, uint32_t* to) {
    const uint32_t f = e / 3u, c = e - 3u * f, d = c == 2u ? 0u : c + 1u;
    *from = (uint32_t)face[3 * (int64_t)f + c]; *to = (uint32_t)face[3 * (int64_t)f + d];
}

// one thread per face: validity, the face's own union-find word, its three edge uses
__global__ __launch_bounds__(WG) void topo_insert_kernel(TopoArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool ignored = false;
    if (f < a.F) {
        const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
        const bool ok = dudf_face_in_range(i0, i1, i2, a.V) && i0 != i1 && i1 != i2 && i2 != i0;
        a.valid[f] = ok ? 1 : 0;
        a.pp[0][f] = (uint32_t)f << 1;                           // every face its own root, parity 0
        ignored = !ok;
        if (ok) {
            const uint32_t idx[3] = {(uint32_t)i0, (uint32_t)i1, (uint32_t)i2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t e = 3u * (uint32_t)f + (uint32_t)c;
                const int64_t s = dudf_edge_claim(a.etab, a.cap, dudf_edge_key(idx[c], idx[c == 2 ? 0 : c + 1]));
                if (s >= 0) { atomicAdd(&a.ecnt[s], 1u); atomicMin(&a.emin[s], e); atomicMax(&a.emax[s], e); }
            }
        }
    }
    unsigned total;
    dudf_wg_rank(ignored, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_IGNORED, total);
}

// one thread per face-slot: its partner over a manifold edge and the relative sign; the edge classes, each edge counted once (by
// its smallest face-slot)
__global__ __launch_bounds__(WG) void topo_resolve_kernel(TopoArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t e = dudf_wg_item();
    bool border = false, manifold = false, fin = false;
    if (e < 3 * a.F) {
        uint32_t l = NONE32;
        if (a.valid[e / 3]) {
            uint32_t from, to;
            slot_edge(a.face, (uint32_t)e, &from, &to);
            const int64_t s = dudf_edge_slot(a.etab, a.cap, dudf_edge_key(from, to));
            if (s >= 0) {
                const uint32_t n = a.ecnt[s], lo = a.emin[s], hi = a.emax[s];
                const bool first = lo == (uint32_t)e;
                border = n == 1u; manifold = n == 2u && first; fin = n > 2u && first;
                const uint32_t p = first ? hi : lo;
                if (n == 2u && lo != hi && p < 3 * a.F && (first || hi == (uint32_t)e)) {
                    uint32_t pf, pt;
                    slot_edge(a.face, p, &pf, &pt);
                    l = p | (((from < to) == (pf < pt)) ? SAME_BIT : 0u);
                }
            }
        }
        a.link[e] = l;
    }
    unsigned total;
    dudf_wg_rank(border, wt, &total);   dudf_wg_add_total(a.ctr + CTR_BORDER, total);
    dudf_wg_rank(manifold, wt, &total); dudf_wg_add_total(a.ctr + CTR_MANIFOLD, total);
    dudf_wg_rank(fin, wt, &total);      dudf_wg_add_total(a.ctr + CTR_NONMANIFOLD, total);
}

// one thread per face-slot; a link is handled by its smaller face-slot.  pp is flat: the parent is the representative
__global__ __launch_bounds__(WG) void topo_best_kernel(TopoArgs a, const uint32_t* __restrict__ pp) {
    const int64_t e = dudf_wg_item();
    if (e >= 3 * a.F) return;
    const uint32_t l = a.link[e];
    if (l == NONE32) return;
    const uint32_t p = l & ~SAME_BIT;
    if ((uint32_t)e > p) return;
    const uint32_t ra = pp[e / 3] >> 1, rb = pp[p / 3u] >> 1;
    if (ra == rb || ra >= a.F || rb >= a.F) return;
    uint32_t from, to;
    slot_edge(a.face, (uint32_t)e, &from, &to);
    const unsigned long long key = dudf_edge_key(from, to);
    atomicMin(&a.best[ra], key);
    atomicMin(&a.best[rb], key);
}

// every representative with an outgoing link hooks to the other end's representative, except the smaller one of a mutual pair;
// cur -> nxt for every face (the others are copied)
__global__ __launch_bounds__(WG) void topo_hook_kernel(TopoArgs a, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt) {
    __shared__ unsigned wt[WG / 64];
    const int64_t v = dudf_wg_item();
    bool hooked = false;
    if (v < a.F) {
        uint32_t word = cur[v];
        const unsigned long long key = a.best[v];
        if ((word >> 1) == (uint32_t)v && key != kTabEmpty64) {
            const int64_t s = dudf_edge_slot(a.etab, a.cap, key);
            if (s >= 0) {
                const uint32_t ea = a.emin[s], eb = a.emax[s];
                if (ea < 3 * a.F && eb < 3 * a.F) {
                    const uint32_t wi = cur[ea / 3u], wj = cur[eb / 3u];
                    const uint32_t ri = wi >> 1, rj = wj >> 1;
                    const uint32_t other = ri == (uint32_t)v ? rj : ri;
                    if (other < a.F && other != (uint32_t)v && !(a.best[other] == key && (uint32_t)v < other)) {
                        const uint32_t sign = a.link[ea] >> 31;          // same direction: one of the two has to turn
                        word = (other << 1) | ((wi ^ wj ^ sign) & 1u);
                        hooked = true;
                    }
                }
            }
        }
        nxt[v] = word;
    }
    unsigned total;
    dudf_wg_rank(hooked, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_FOREST, total);
}

// one pointer-doubling step cur -> nxt of (parent, parity); flags[step] says whether anything moved, and a step whose predecessor
// moved nothing returns at once (both buffers are then equal)
__global__ __launch_bounds__(WG) void topo_jump_kernel(int64_t F, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt,
                                                       unsigned* __restrict__ flags, int step) {
    if (step > 0 && flags[step - 1] == 0u) return;
    const int64_t v = dudf_wg_item();
    bool moved = false;
    if (v < F) {
        const uint32_t w = cur[v], p = w >> 1;
        uint32_t o = w;
        if (p < F) {
            const uint32_t b = cur[p];
            o = (b & ~1u) | ((w ^ b) & 1u);
        }
        nxt[v] = o;
        moved = o != w;
    }
    if (__any(moved) && (threadIdx.x & 63) == 0) atomicOr(&flags[step], 1u);
}

__global__ __launch_bounds__(WG) void topo_label_kernel(TopoArgs a, const uint32_t* __restrict__ pp) {
    const int64_t v = dudf_wg_item();
    if (v >= a.F) return;
    const uint32_t r = pp[v] >> 1;
    if (r < a.F) atomicMin(&a.label[r], (uint32_t)v);
}

// q = (uint64) rint(min(nn, 16) * 2^30) of a valid face, nn as in dudf_surfsample.hip; a non-finite nn: 0
__device__ __forceinline__ unsigned long long face_area_q(const double* __restrict__ v, int64_t i0, int64_t i1, int64_t i2) {
    const double e0 = v[i1 * 3] - v[i0 * 3], e1 = v[i1 * 3 + 1] - v[i0 * 3 + 1], e2 = v[i1 * 3 + 2] - v[i0 * 3 + 2];
    const double g0 = v[i2 * 3] - v[i0 * 3], g1 = v[i2 * 3 + 1] - v[i0 * 3 + 1], g2 = v[i2 * 3 + 2] - v[i0 * 3 + 2];
    const double n0 = e1 * g2 - e2 * g1, n1 = e2 * g0 - e0 * g2, n2 = e0 * g1 - e1 * g0;
    const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (!(nn <= 1.79769313486231570815e308)) return 0ull;
    return (unsigned long long)__builtin_rint((nn < 16.0 ? nn : 16.0) * 1073741824.0);
}

// one thread per face: label, flip relative to the label face, the oriented face, the component's face count and area
__global__ __launch_bounds__(WG) void topo_write_kernel(TopoArgs a, const uint32_t* __restrict__ pp, int64_t* __restrict__ out_faces,
                                                        int64_t* __restrict__ out_component, uint8_t* __restrict__ out_flip,
                                                        unsigned long long* __restrict__ out_nfaces, unsigned long long* __restrict__ out_area) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool flipped = false, is_label = false;
    if (f < a.F) {
        const uint32_t w = pp[f], r = w >> 1;
        uint32_t lab = r < a.F ? a.label[r] : (uint32_t)f;
        if (lab >= a.F) lab = (uint32_t)f;
        const uint32_t flip = (w ^ pp[lab]) & 1u;                 // both parities are relative to the same representative
        const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
        out_faces[3 * f] = i0; out_faces[3 * f + 1] = flip ? i2 : i1; out_faces[3 * f + 2] = flip ? i1 : i2;
        out_component[f] = lab; out_flip[f] = (uint8_t)flip;
        atomicAdd(&out_nfaces[lab], 1ull);
        if (a.vert && a.valid[f]) {
            const unsigned long long q = face_area_q(a.vert, i0, i1, i2);
            if (q) atomicAdd(&out_area[lab], q);
        }
        flipped = flip != 0u; is_label = lab == (uint32_t)f;
    }
    unsigned total;
    dudf_wg_rank(flipped, wt, &total);  dudf_wg_add_total(a.ctr + CTR_FLIPPED, total);
    dudf_wg_rank(is_label, wt, &total); dudf_wg_add_total(a.ctr + CTR_COMPONENTS, total);
}

// one thread per face-slot: the manifold edges both faces still traverse the same way
__global__ __launch_bounds__(WG) void topo_inconsistent_kernel(TopoArgs a, const uint8_t* __restrict__ flip) {
    __shared__ unsigned wt[WG / 64];
    const int64_t e = dudf_wg_item();
    bool bad = false;
    if (e < 3 * a.F) {
        const uint32_t l = a.link[e];
        if (l != NONE32) {
            const uint32_t p = l & ~SAME_BIT;
            if ((uint32_t)e < p && p < 3 * a.F) bad = (((l >> 31) ^ flip[e / 3] ^ flip[p / 3u]) & 1u) != 0u;
        }
    }
    unsigned total;
    dudf_wg_rank(bad, wt, &total);
    dudf_wg_add_total(a.ctr + CTR_INCONSISTENT, total);
}

__global__ void topo_finish_kernel(const unsigned long long* __restrict__ ctr, int64_t* __restrict__ out_counts) {
    if (threadIdx.x < N_CTR && blockIdx.x == 0) out_counts[threadIdx.x] = (int64_t)ctr[threadIdx.x];
}

int ceil_log2(int64_t n) { int b = 0; while (((int64_t)1 << b) < n) ++b; return b; }
bool topo_sizes_ok(int64_t F) { return F >= 0 && 6 * F < (1ll << 32); }

// zero-initialised arrays first, 0xff-initialised second, the rest behind (dudf_init_spans)
DudfSpans carve_topo(void* ws, int64_t F, TopoArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    a->F = F; a->cap = dudf_pow2_at_least(6 * F);
    a->ctr = cv.take<unsigned long long>(N_CTR); a->flags = cv.take<unsigned>(64);
    a->ecnt = cv.take<uint32_t>(a->cap); a->emax = cv.take<uint32_t>(a->cap);
    DudfSpans sp;
    sp.zero_end = sp.ff_begin = cv.o;
    a->etab = cv.take<unsigned long long>(a->cap); a->emin = cv.take<uint32_t>(a->cap); a->label = cv.take<uint32_t>(F);
    sp.ff_end = cv.o;
    a->pp[0] = cv.take<uint32_t>(F); a->pp[1] = cv.take<uint32_t>(F); a->best = cv.take<unsigned long long>(F);
    a->link = cv.take<uint32_t>(3 * F); a->valid = cv.take<uint8_t>(F);
    sp.total = cv.o;
    return sp;
}

// ---------------------------------------------------------------------------------------------------------------- submesh by mask
struct SubArgs {
    const double* vert; const int64_t* face; const uint8_t* keep; int64_t V, F, nbV, nbF;
    int64_t* head;                       // [3] magic, V, F: what the workspace holds (emit checks it on the device)
    int64_t* tot;                        // [2] V', F'
    uint8_t* vuse;                       // [V] a kept face uses the vertex
    int32_t* vnew;                       // [V] index after compaction
    uint8_t* fkeep;                      // [F] kept and every index in range
    uint32_t* vblk; int64_t* voff;       // [nbV]
    uint32_t* fblk; int64_t* foff;       // [nbF]
    double* out_v; int64_t* out_f;
};

__global__ __launch_bounds__(WG) void sub_mark_kernel(SubArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t f = dudf_wg_item();
    bool k = false;
    if (f < a.F) {
        const int64_t i0 = a.face[3 * f], i1 = a.face[3 * f + 1], i2 = a.face[3 * f + 2];
        k = a.keep[f] != 0 && dudf_face_in_range(i0, i1, i2, a.V);
        a.fkeep[f] = k ? 1 : 0;
        if (k) { a.vuse[i0] = 1; a.vuse[i1] = 1; a.vuse[i2] = 1; }
    }
    unsigned total;
    dudf_wg_rank(k, wt, &total);
    if (threadIdx.x == 0) a.fblk[blockIdx.x] = total;
}

__global__ __launch_bounds__(WG) void sub_vertices_kernel(SubArgs a) {
    __shared__ unsigned wt[WG / 64];
    const int64_t v = dudf_wg_item();
    unsigned total;
    dudf_wg_rank(v < a.V && a.vuse[v], wt, &total);
    if (threadIdx.x == 0) a.vblk[blockIdx.x] = total;
}

__global__ void sub_finish_kernel(SubArgs a, int64_t* out_counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out_counts[0] = a.tot[0]; out_counts[1] = a.tot[1];
    a.head[0] = MAGIC_SUBMESH; a.head[1] = a.V; a.head[2] = a.F;
}

// V == 0 or F == 0: nothing survives
__global__ void sub_empty_kernel(int64_t* out_counts, int64_t* head) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out_counts[0] = 0; out_counts[1] = 0; head[0] = 0;
}

__device__ __forceinline__ bool sub_head_ok(const SubArgs& a) { return a.head[0] == MAGIC_SUBMESH && a.head[1] == a.V && a.head[2] == a.F; }

__global__ __launch_bounds__(WG) void sub_emit_vertices_kernel(SubArgs a) {
    __shared__ unsigned wt[WG / 64];
    if (!sub_head_ok(a)) return;                                         // uniform: the whole grid leaves
    const int64_t v = dudf_wg_item();
    const bool use = v < a.V && a.vuse[v];
    unsigned total;
    const unsigned r = dudf_wg_rank(use, wt, &total);
    if (use) {
        const int64_t n = a.voff[blockIdx.x] + r;
        a.vnew[v] = (int32_t)n;
        a.out_v[3 * n] = a.vert[3 * v]; a.out_v[3 * n + 1] = a.vert[3 * v + 1]; a.out_v[3 * n + 2] = a.vert[3 * v + 2];
    }
}

__global__ __launch_bounds__(WG) void sub_emit_faces_kernel(SubArgs a) {
    __shared__ unsigned wt[WG / 64];
    if (!sub_head_ok(a)) return;
    const int64_t f = dudf_wg_item();
    const bool k = f < a.F && a.fkeep[f];
    unsigned total;
    const unsigned r = dudf_wg_rank(k, wt, &total);
    if (k) {
        const int64_t n = a.foff[blockIdx.x] + r;
        a.out_f[3 * n] = a.vnew[a.face[3 * f]]; a.out_f[3 * n + 1] = a.vnew[a.face[3 * f + 1]]; a.out_f[3 * n + 2] = a.vnew[a.face[3 * f + 2]];
    }
}

bool sub_sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < (1ll << 31) && F < (1ll << 31); }

DudfSpans carve_sub(void* ws, int64_t V, int64_t F, SubArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    a->V = V; a->F = F; a->nbV = dudf_wg_count(V); a->nbF = dudf_wg_count(F);
    a->head = cv.take<int64_t>(3); a->tot = cv.take<int64_t>(2); a->vuse = cv.take<uint8_t>(V);
    DudfSpans sp;
    sp.zero_end = sp.ff_begin = sp.ff_end = cv.o;                       // no table here
    a->vnew = cv.take<int32_t>(V); a->fkeep = cv.take<uint8_t>(F);
    a->vblk = cv.take<uint32_t>(a->nbV); a->voff = cv.take<int64_t>(a->nbV);
    a->fblk = cv.take<uint32_t>(a->nbF); a->foff = cv.take<int64_t>(a->nbF);
    sp.total = cv.o;
    return sp;
}

int fill_sub(int64_t V, const int64_t* faces, int64_t F, const uint8_t* keep, void* ws, size_t bytes, SubArgs* a, DudfSpans* sp) {
    if (V < 0 || F < 0) return DUDF_E_BADCFG;
    if (!sub_sizes_ok(V, F)) return DUDF_E_UNSUPPORTED;
    if (F > 0 && (!faces || !keep)) return DUDF_E_BADCFG;
    *sp = carve_sub(ws, V, F, a);
    if (int rc = dudf_check_buffer(ws, bytes, sp->total)) return rc;
    a->vert = nullptr; a->face = faces; a->keep = keep; a->out_v = nullptr; a->out_f = nullptr;
    return 0;
}

}  // namespace

extern "C" {

size_t dudf_mesh_topology_workspace_bytes(int64_t F) {
    if (!topo_sizes_ok(F)) return 0;
    TopoArgs a;
    return carve_topo(nullptr, F, &a).total;
}

int dudf_mesh_topology(const int64_t* faces, int64_t F, int64_t V, const double* vertices, int64_t* out_faces, int64_t* out_component,
                       unsigned char* out_flip, int64_t* out_component_faces, uint64_t* out_component_area_q, int64_t* out_counts,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (F < 0 || V < 0) return DUDF_E_BADCFG;
    if (!topo_sizes_ok(F) || V >= (1ll << 31)) return DUDF_E_UNSUPPORTED;
    if (!out_counts) return DUDF_E_BADCFG;
    if (F > 0 && (!faces || !out_faces || !out_component || !out_flip || !out_component_faces || !out_component_area_q)) return DUDF_E_BADCFG;
    if (F > 0 && out_faces == faces) return DUDF_E_BADCFG;           // every round re-reads the directions from the input
    TopoArgs a;
    const DudfSpans sp = carve_topo(workspace, F, &a);
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, sp.total)) return rc;
    a.face = faces; a.vert = vertices; a.V = V;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    if (F == 0) return (int)hipMemsetAsync(out_counts, 0, N_CTR * sizeof(int64_t), st);
    DUDF_TRY(dudf_init_spans(workspace, sp, st));
    DUDF_TRY(hipMemsetAsync(out_component_faces, 0, (size_t)F * sizeof(int64_t), st));
    DUDF_TRY(hipMemsetAsync(out_component_area_q, 0, (size_t)F * sizeof(uint64_t), st));
    const dim3 gf((unsigned)dudf_wg_count(F)), gs((unsigned)dudf_wg_count(3 * F)), wg(WG);
    DUDF_TRY(dudf_launch(topo_insert_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(topo_resolve_kernel, gs, wg, st, a));
    // Borůvka: the components at least halve per round that hooks anything, and a round that hooks nothing is the last
    const int jumps = ceil_log2(F) > 0 ? ceil_log2(F) : 1, max_rounds = ceil_log2(F) + 1;
    int c = 0;                                                       // pp[c] is current and flat
    unsigned long long total_hooks = 0;
    for (int r = 0; r < max_rounds; ++r) {
        DUDF_TRY(hipMemsetAsync(a.best, 0xff, (size_t)F * sizeof(unsigned long long), st));
        DUDF_TRY(hipMemsetAsync(a.flags, 0, 64 * sizeof(unsigned), st));
        DUDF_TRY(dudf_launch(topo_best_kernel, gs, wg, st, a, (const uint32_t*)a.pp[c]));
        DUDF_TRY(dudf_launch(topo_hook_kernel, gf, wg, st, a, (const uint32_t*)a.pp[c], a.pp[1 - c]));
        c = 1 - c;
        for (int s = 0; s < jumps; ++s) {
            DUDF_TRY(dudf_launch(topo_jump_kernel, gf, wg, st, F, (const uint32_t*)a.pp[c], a.pp[1 - c], a.flags, s));
            c = 1 - c;
        }
        unsigned long long hooks = 0;                                // the one read-back of the round
        DUDF_TRY(hipMemcpyAsync(&hooks, a.ctr + CTR_FOREST, sizeof(hooks), hipMemcpyDeviceToHost, st));
        DUDF_TRY(hipStreamSynchronize(st));
        if (hooks == total_hooks) break;
        total_hooks = hooks;
    }
    DUDF_TRY(dudf_launch(topo_label_kernel, gf, wg, st, a, (const uint32_t*)a.pp[c]));
    DUDF_TRY(dudf_launch(topo_write_kernel, gf, wg, st, a, (const uint32_t*)a.pp[c], out_faces, out_component, (uint8_t*)out_flip,
                         reinterpret_cast<unsigned long long*>(out_component_faces),
                         reinterpret_cast<unsigned long long*>(out_component_area_q)));
    DUDF_TRY(dudf_launch(topo_inconsistent_kernel, gs, wg, st, a, (const uint8_t*)out_flip));
    return dudf_launch(topo_finish_kernel, dim3(1), dim3(64), st, (const unsigned long long*)a.ctr, out_counts);
}

size_t dudf_mesh_submesh_workspace_bytes(int64_t V, int64_t F) {
    if (!sub_sizes_ok(V, F)) return 0;
    SubArgs a;
    return carve_sub(nullptr, V, F, &a).total;
}

int dudf_mesh_submesh_count(int64_t V, const int64_t* faces, int64_t F, const unsigned char* keep, int64_t* out_counts, void* workspace,
                            size_t workspace_bytes, void* stream) {
    SubArgs a; DudfSpans sp;
    int rc = fill_sub(V, faces, F, keep, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if (!out_counts) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    if (V == 0 || F == 0) return dudf_launch(sub_empty_kernel, dim3(1), dim3(1), st, out_counts, a.head);
    DUDF_TRY(dudf_init_spans(workspace, sp, st));
    const dim3 gv((unsigned)a.nbV), gf((unsigned)a.nbF), wg(WG);
    DUDF_TRY(dudf_launch(sub_mark_kernel, gf, wg, st, a));
    DUDF_TRY(dudf_launch(sub_vertices_kernel, gv, wg, st, a));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, a.vblk, a.voff, a.nbV, a.tot));
    DUDF_TRY(dudf_launch(dudf_scan_totals_kernel<1>, dim3(1), dim3(1024), st, a.fblk, a.foff, a.nbF, a.tot + 1));
    return dudf_launch(sub_finish_kernel, dim3(1), dim3(1), st, a, out_counts);
}

int dudf_mesh_submesh_emit(const double* vertices, int64_t V, const int64_t* faces, int64_t F, const unsigned char* keep,
                           double* out_vertices, int64_t* out_faces, void* workspace, size_t workspace_bytes, void* stream) {
    SubArgs a; DudfSpans sp;
    int rc = fill_sub(V, faces, F, keep, workspace, workspace_bytes, &a, &sp);
    if (rc) return rc;
    if ((V > 0 && !vertices) || !out_vertices || !out_faces) return DUDF_E_BADCFG;
    if (V == 0 || F == 0) return 0;
    a.vert = vertices; a.out_v = out_vertices; a.out_f = out_faces;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const dim3 gv((unsigned)a.nbV), gf((unsigned)a.nbF), wg(WG);
    DUDF_TRY(dudf_launch(sub_emit_vertices_kernel, gv, wg, st, a));
    return dudf_launch(sub_emit_faces_kernel, gf, wg, st, a);
}

}  // extern "C"
