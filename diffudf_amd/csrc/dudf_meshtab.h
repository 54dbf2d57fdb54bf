// The hash tables of the mesh units (clean-up, topology, simplification), stated once (DESIGN.md §3 "Mesh clean-up").  Device code with
// the few host helpers that go with it.  Internal: not installed, nothing here is part of the C ABI.
//
// The rules every table here keeps:
//   - open addressing with linear probing from mix64(key) & (cap - 1); the capacity is a power of two of at least twice the items;
//   - nothing is ever deleted, so a probe chain ends at the key or at the first empty slot;
//   - every loop is bounded by the capacity: a table that is full, or was not built by this call, ends the loop instead of hanging it;
//   - keys are compared by recomputing them from immutable input (the caller's arrays, or what the launch before wrote): no thread
//     waits for, or reads, what another thread of the same launch writes beside the slot word.
// Two tables:
//   edges           a slot holds the key itself, (min << 32 | max), claimed with a 64-bit atomicCAS.  The helpers return the SLOT; what
//                   a unit keeps per edge (use counts, a direction bit, the smallest and largest user) lives in its own arrays beside
//                   the table, under its own atomics;
//   smallest index  a slot holds the index of SOME item with the slot's key, claimed with atomicCAS and lowered with atomicMin: it
//                   ends as the smallest index with that key, whatever the arrival order.  An item set states key(i), same and hash.
// Empty slots are all ones: one 0xff memset (dudf_init_spans) clears both kinds.
#pragma once
#include "dudf_context.h"
#include "dudf_wgscan.h"

constexpr uint32_t kTabEmpty32 = 0xffffffffu;
constexpr unsigned long long kTabEmpty64 = ~0ull;

__device__ __forceinline__ uint64_t dudf_mix64(uint64_t x) {  // splitmix64's finaliser: lattice keys must not cluster
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// ---- edge table ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long dudf_edge_key(uint32_t u, uint32_t w) {        // undirected: (min << 32 | max)
    return u < w ? ((unsigned long long)u << 32) | w : ((unsigned long long)w << 32) | u;
}
// the slot that holds `key` from now on, claimed if no thread had yet; -1: the table is full (the caller skips the edge)
__device__ __forceinline__ int64_t dudf_edge_claim(unsigned long long* __restrict__ etab, int64_t cap, unsigned long long key) {
    int64_t s = (int64_t)(dudf_mix64(key) & (uint64_t)(cap - 1));
    for (int64_t i = 0; i < cap; ++i, s = (s + 1) & (cap - 1)) {
        const unsigned long long cur = atomicCAS(&etab[s], kTabEmpty64, key);
        if (cur == kTabEmpty64 || cur == key) return s;
    }
    return -1;
}
// the slot of a key the table holds, -1 otherwise (table complete: read only)
__device__ __forceinline__ int64_t dudf_edge_slot(const unsigned long long* __restrict__ etab, int64_t cap, unsigned long long key) {
    int64_t s = (int64_t)(dudf_mix64(key) & (uint64_t)(cap - 1));
    for (int64_t i = 0; i < cap; ++i, s = (s + 1) & (cap - 1)) {
        const unsigned long long cur = etab[s];
        if (cur == key) return s;
        if (cur == kTabEmpty64) return -1;
    }
    return -1;
}

// ---- smallest-index table --------------------------------------------------------------------------------------------------------
// Items: `Key key(int64_t i) const`, `static bool same(Key, Key)`, `static uint64_t hash(Key)`.  n: the items; a slot word that is no
// item (a table this call did not build) is never turned into a key.
// enters item i; true when this thread claimed an empty slot (once per distinct key)
template <class Items>
__device__ __forceinline__ bool dudf_first_insert(uint32_t* __restrict__ tab, int64_t cap, const Items& items, int64_t i, int64_t n) {
    const auto k = items.key(i);
    int64_t s = (int64_t)(Items::hash(k) & (uint64_t)(cap - 1));
    for (int64_t t = 0; t < cap; ++t, s = (s + 1) & (cap - 1)) {
        const uint32_t cur = atomicCAS(&tab[s], kTabEmpty32, (uint32_t)i);
        if (cur == kTabEmpty32) return true;
        if (cur < n && Items::same(items.key(cur), k)) { atomicMin(&tab[s], (uint32_t)i); return false; }
    }
    return false;
}
// the smallest item with key k, kTabEmpty32 when the table holds none (table complete: read only)
template <class Items, class Key>
__device__ __forceinline__ uint32_t dudf_first_find(const uint32_t* __restrict__ tab, int64_t cap, const Items& items, const Key& k, int64_t n) {
    int64_t s = (int64_t)(Items::hash(k) & (uint64_t)(cap - 1));
    for (int64_t t = 0; t < cap; ++t, s = (s + 1) & (cap - 1)) {
        const uint32_t cur = tab[s];
        if (cur == kTabEmpty32) break;
        if (cur < n && Items::same(items.key(cur), k)) return cur;
    }
    return kTabEmpty32;
}

// the faces of g[F][3] by their vertex SET: the sorted triple
struct DudfTri { int32_t a, b, c; };                          // a <= b <= c
struct DudfTriItems {
    const int32_t* g;
    __device__ __forceinline__ DudfTri key(int64_t f) const {
        int32_t a = g[3 * f], b = g[3 * f + 1], c = g[3 * f + 2], t;
        if (a > b) { t = a; a = b; b = t; }
        if (b > c) { t = b; b = c; c = t; }
        if (a > b) { t = a; a = b; b = t; }
        return DudfTri{a, b, c};
    }
    __device__ __forceinline__ static bool same(const DudfTri& p, const DudfTri& q) { return p.a == q.a && p.b == q.b && p.c == q.c; }
    __device__ __forceinline__ static uint64_t hash(const DudfTri& k) {
        return dudf_mix64(dudf_mix64(((uint64_t)(uint32_t)k.a << 32) | (uint32_t)k.b) ^ (uint32_t)k.c);
    }
};

// ---- face validity ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dudf_face_in_range(int64_t i0, int64_t i1, int64_t i2, int64_t V) {
    return i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
}
// all nine coordinates finite.  It reads them: call it only behind the range check (`in_range && finite`)
__device__ __forceinline__ bool dudf_face_finite(const double* __restrict__ vert, int64_t i0, int64_t i1, int64_t i2) {
    const int64_t idx[3] = {i0, i1, i2};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) ok = ok && isfinite(vert[3 * idx[k] + c]);
    return ok;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline int64_t dudf_pow2_at_least(int64_t n) { int64_t c = 2; while (c < n) c <<= 1; return c; }
inline int64_t dudf_wg_count(int64_t n) { return (n + DUDF_WG - 1) / DUDF_WG; }        // workgroups of n items, one thread each

// What a carve_* function says of its layout: [0, zero_end) starts as zeros, [ff_begin, ff_end) as empty slots, the rest is written
// before it is read; total: the workspace's bytes.  A workspace without tables has ff_begin == ff_end.
struct DudfSpans { size_t zero_end, ff_begin, ff_end, total; };
inline int dudf_init_spans(void* ws, const DudfSpans& sp, hipStream_t st) {
    char* base = static_cast<char*>(ws);
    DUDF_TRY(hipMemsetAsync(base, 0, sp.zero_end, st));
    if (sp.ff_end > sp.ff_begin) DUDF_TRY(hipMemsetAsync(base + sp.ff_begin, 0xff, sp.ff_end - sp.ff_begin, st));
    return 0;
}
