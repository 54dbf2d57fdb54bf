// The nearest-primitive walk of dudf_meshdist.hip (walk_nearest) with the two remedies its measurements asked for:
// kGwSplit = 8 adjacent lanes of one wave share one query — the sampler's QSPLIT, and the index's 8 primitives per leaf — so
//   - a leaf is ONE step: lane j loads primitive j of the leaf (288 contiguous bytes of triangles, 128 of points), evaluates it
//     exactly, and the group takes the minimum with three __shfl_xor (1, 2, 4);
//   - a wave carries 8 queries instead of 64, so eight times as many waves hide each other's dependent box loads.
// The walk is UNIFORM across a group: node, stack pointer and bound are functions of the query and of the group minimum, which
// all eight lanes hold alike.  Every lane writes the group's stack entry (the same value to the same LDS word) and reads back
// what it wrote itself, so no lane depends on another's store; the only cross-lane traffic is the shuffles, whose partners take
// the same branch.  No barrier; every node is entered at most once, so the walk ends whatever the numbers are.
//
// Internal step and pruning are walk_nearest's: nearer child first; a subtree is skipped only on the safe-side test of dudf_bvh.h
// (box_lb > bound_of), on meeting the node and again on popping it.  The result is the minimum of exact fp64 values over a set that
// contains every minimiser — a number that does not depend on the order of visits — so it is the brute-force scan's bit for bit.
// Only the value is kept, not who attains it.
//
// The tree is the fixed-shape one of dudf_bvh.h, which two indexes have: the mesh index (leaves of 8 sorted triangles, 9 floats
// each) and the cloud index (leaves of 8 sorted points as 16-byte rows).
#ifndef DUDF_GROUPWALK_H
#define DUDF_GROUPWALK_H
#include "dudf_bvh.h"
#include "dudf_tridist.h"

constexpr int kGwSplit = kBvhLeaf;                    // lanes per query = primitives per leaf
constexpr int kGwBlock = 256;                         // threads per workgroup
constexpr int kGwGroups = kGwBlock / kGwSplit;        // queries per workgroup
static_assert(64 % kGwSplit == 0, "a group lies inside one wave");

struct GwTree {                       // what a walk reads
    const float4* nodes; const void* prims;
    int64_t n; int L, depth;
};
inline size_t gw_lds_bytes(const GwTree& t) { return (size_t)t.depth * kGwGroups * (sizeof(int) + sizeof(float)); }   // <= 29 * 256 bytes

// ---- leaf evaluators: the exact squared distance from p to primitive s ------------------------------------------------------------
struct GwTriLeaf {                    // sorted triangles [n][9]: the Voronoi-region arithmetic every distance kernel uses
    static __device__ __forceinline__ double eval(const void* prims, int64_t s, double px, double py, double pz) {
        return tri_dist2(px, py, pz, static_cast<const float*>(prims) + s * 9);
    }
};
struct GwPointLeaf {                  // sorted points [n] float4: the expression of sample_batch_kernel's cloud branch, products unfused
    static __device__ __forceinline__ double eval(const void* prims, int64_t s, double px, double py, double pz) {
#pragma clang fp contract(off)
        const float4 q = static_cast<const float4*>(prims)[s];
        const double dx = px - q.x, dy = py - q.y, dz = pz - q.z;
        return dx * dx + dy * dy + dz * dz;
    }
};

// The minimum over all primitives of Leaf::eval for the query (fx, fy, fz) the kGwSplit lanes of a group share; `part` = this
// lane's place in its group; snode / slb: the group's column of the [entry][group] stacks (entry e at [e * kGwGroups]).  Called by
// all lanes of a group or by none.  evals += this lane's exact evaluations.  `best`: the value the caller's scan starts from — the
// result when no evaluation is below it (a NaN evaluation never is), so that even then walk and scan agree; it must be an upper
// bound that every lane of the group passes alike, +inf when in doubt.
template <class Leaf>
__device__ __forceinline__ double gw_walk_nearest(const GwTree& t, int* snode, float* slb, float fx, float fy, float fz, int part,
                                                  double best, unsigned long long& evals) {
    const double px = fx, py = fy, pz = fz;
    float bestf = bound_of(best);
    const int first_leaf = t.L - 1;
    int node = 0, sp = 0;
    for (;;) {
        bool pop = true;
        if (node >= first_leaf) {
            const int64_t s = (int64_t)(node - first_leaf) * kGwSplit + part;
            double d2 = __builtin_inf();
            if (s < t.n) { d2 = Leaf::eval(t.prims, s, px, py, pz); ++evals; }
#pragma unroll
            for (int m = 1; m < kGwSplit; m <<= 1) d2 = fmin(d2, __shfl_xor(d2, m));
            if (d2 < best) best = d2;
            bestf = bound_of(best);
        } else {
            const float4* c = t.nodes + 2 * (2 * (int64_t)node + 1);
            const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
            float ln = box_lb(l0, l1, fx, fy, fz), lf = box_lb(r0, r1, fx, fy, fz);
            int nn = 2 * node + 1, nf = nn + 1;
            if (lf < ln) { const float s = ln; ln = lf; lf = s; nn = nf; nf = nn - 1; }
            if (!(ln > bestf)) {                  // the nearer child may hold the answer; the farther one waits on the stack
                if (!(lf > bestf)) { snode[sp * kGwGroups] = nf; slb[sp * kGwGroups] = lf; ++sp; }
                node = nn; pop = false;
            }
        }
        if (pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                if (!(slb[sp * kGwGroups] > bestf)) { node = snode[sp * kGwGroups]; found = true; break; }
            }
            if (!found) break;
        }
    }
    return best;
}

#endif  // DUDF_GROUPWALK_H
