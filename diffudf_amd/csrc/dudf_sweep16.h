// Pieces shared by the three translation units of the SIREN sweeps on the 16-bit matrix cores (gfx950 / CDNA4):
// dudf_sweep_bf16.hip (128- and 256-wide layers), dudf_sweep_wide.hip (512-wide layers) and dudf_prep.hip (the kernels that
// write the weight images).  All three rest on the operand split and on the A-fragment image described here.
//
// A hidden layer  OUT[feature][column] = M[feature][k] * IN[k][column]  is multiplied like this ("bf16x6"):
// every fp32 operand is split EXACTLY into three bf16 pieces v = h + m + l (8+8+8 significand bits,
// round-to-nearest at each step so the three pieces always hold all 24 bits); a product is the six partial products
// whose weight is >= 2^-16 (hh, hm, mh, hl, lh, mm — the dropped ml, lm, ll are below fp32 rounding), accumulated in
// fp32 by v_mfma_f32_16x16x32_bf16.  Six of those (16 cycles each, K = 32) replace eight v_mfma_f32_16x16x4_f32
// (32 cycles each, K = 4): 96 instead of 256 matrix-core cycles per 16x16 tile and 32 features.
// ("fp16x3", the two-piece fp16 split with three products: see GeoB below.)
//
// The weights are pre-split once per step (pack kernels, dudf_prep.hip) into an image in A-FRAGMENT ORDER: for every
// (k-block, 16-row tile, piece) the 1 KiB that one ds_read_b128 wave-instruction fetches, lane L = (g<<4 | m)
// holding M[row m][the 8 features of k-slots (g, 0..7)] (k-slot (g, e) of k-block kb is feature 32kb + 4g + e for e < 4,
// 32kb + 16 + 4g + (e-4) otherwise: the mapping in dudf_sweep_bf16.hip).  The 48 KiB of a k-block (16 tiles x 3 pieces at
// H = 256) are contiguous, so LDS-DMA moves them verbatim in 1 KiB wave-instructions and the reads are lane-linear:
// conflict-free without padding or swizzle.
//
// Everything below sits in the anonymous namespace: each unit gets its own copy, and the kernels keep their names.  That holds
// for the debug state too: the DUDF_FX_CHECK counters of dudf_sweep_common.h exist once per unit (dudf_fx_read below).
#pragma once
#include "dudf_sweep_common.h"
#include <type_traits>

namespace {

// one LDS atomic per wave: 64 lanes hitting the same LDS word serialise (measured: the per-layer publish of the quads' forward
// sweep cost 0.09 ms per launch that way), so the wave reduces first
__device__ __forceinline__ void lds_max_wave(unsigned* word, float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    // lane 0 alone, WITHOUT a compiler-visible branch: `if (lane == 0)` ends the basic block, and the sweeps call this in the last
    // k-block step of every layer — the step then loses the interleaving of its tail with its MFMAs (round 5: the same shape of store
    // cost the reverse sweeps 12-18 %, profiles/r05_e_ab.txt)
    const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)word;
    uint64_t ex;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_max_u32 %1, %2\n\ts_mov_b64 exec, %0"
                 : "=&s"(ex) : "v"(addr), "v"(__float_as_uint(v)) : "memory");
}
constexpr int NWB = 8;                                 // waves per workgroup: two per SIMD
constexpr int TILEB = NWB * 16;                        // columns per workgroup pass

// SP = 0: exact three-piece bf16 split, six products ("bf16x6").  SP = 1: fp16 hi/lo split, three products ("fp16x3"):
// v * 2^k = hi + lo with two round-to-nearest fp16 pieces (|v 2^k - hi - lo| <= 2^-23 |v 2^k|; fp16 subnormals are
// produced by v_cvt_pk_f16_f32 and honoured by the MFMA — tools/micro/f16_split.hip, profiles/r03_f16_split_facts.txt),
// products hi*hi + hi*lo + lo*hi; the dropped lo*lo is <= 2^-22 of the product.  Half the matrix-core work, a third less
// LDS traffic, 2 conversions instead of 3 per value; the price is fp16's range: the weights are scaled per matrix by a power
// of two (pack kernel), the activations where their size is not known a priori (see `col_scale`).
template <int H, int SP = 0>
struct GeoB {
    static constexpr int NPC = SP ? 2 : 3;             // pieces per operand
    static constexpr int NT = H / 16;                  // 16-feature tiles per activation vector
    static constexpr int NKB = H / 32;                 // 32-feature k-blocks = weight chunks per layer
    static constexpr int FRAG = 1024;                  // bytes of one A fragment: 64 lanes x 8 x 16 bits
    static constexpr int CHUNKB = NT * NPC * FRAG;     // one k-block of a matrix: [tile][piece]
    static constexpr int IMGB = NKB * CHUNKB;          // one matrix: 6 (4) bytes per weight
    static constexpr int NDMA = NT * NPC / NWB;        // LDS-DMA wave-instructions per wave and chunk
    static constexpr int NTHR = 64 * NWB;
};


__device__ __forceinline__ f32x4 mfma_b(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// 8 fp32 values (two accumulator tiles' registers of one lane) -> the three bf16x8 pieces of a B / A operand
__device__ __forceinline__ void split8(const f32x4 e0, const f32x4 e1, u32x4& h, u32x4& m, u32x4& l) {
    const f32x2 v[4] = {{e0[0], e0[1]}, {e0[2], e0[3]}, {e1[0], e1[1]}, {e1[2], e1[3]}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned hp = cvt_pk(v[i]);
        const f32x2 r1 = v[i] - unpack(hp);                        // exact
        const unsigned mp = cvt_pk(r1);
        const f32x2 r2 = r1 - unpack(mp);                          // exact
        h[i] = hp; m[i] = mp; l[i] = cvt_pk(r2);
    }
}
__device__ __forceinline__ f32x4 mfma_h(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// 8 fp32 values -> the two fp16x8 pieces hi = fp16(v), lo = fp16(v - hi) (the caller has scaled v into fp16's range)
__device__ __forceinline__ void split8h(const f32x4 e0, const f32x4 e1, u32x4& h, u32x4& l) {
    const f32x2 v[4] = {{e0[0], e0[1]}, {e0[2], e0[3]}, {e1[0], e1[1]}, {e1[2], e1[3]}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f16x2 hp = __builtin_convertvector(v[i], f16x2);      // v_cvt_pk_f16_f32, round to nearest even
        // r = v - hi, exact.  v_fma_mix_f32 reads the fp16 half directly (no v_cvt_f32_f16) and issues beside the SIMD
        // partner's MFMAs like a plain v_fma_f32 (tools/micro/coissue.hip); hipcc folds `fma(v, 1, -hi)` back into
        // convert + subtract, hence the asm
        f32x2 r;
        asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r.x) : "v"(v[i].x), "v"(hp));
        asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r.y) : "v"(v[i].y), "v"(hp));
        h[i] = __builtin_bit_cast(unsigned, hp);
        l[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    }
}
__device__ __forceinline__ f16x8 as_h(u32x4 v) { return __builtin_bit_cast(f16x8, v); }
__device__ __forceinline__ bf16x8 as_bf(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ u32x4 as_u(f32x4 v) { return __builtin_bit_cast(u32x4, v); }
__device__ __forceinline__ f32x4 as_f(u32x4 v) { return __builtin_bit_cast(f32x4, v); }

// One chunk of a weight image -> LDS buffer, 1 KiB per wave-instruction (see dudf_sweep.hip for why this is inline asm).
// `lds_off` is the buffer's LDS byte offset, `voff` = lane * 16; this wave moves pieces wave*NDMA .. +NDMA-1.  One asm
// block: scalar base + lane offset addressing, M0 (the LDS destination) saved and restored once — under 2 instructions
// per piece instead of 11 through generic pointers.
template <int H, int SP = 0>
__device__ __forceinline__ void dma_issue(const char* __restrict__ chunk, unsigned lds_off, unsigned voff, int wave) {
    using G = GeoB<H, SP>;
    static_assert(G::NDMA == 6 || G::NDMA == 3 || G::NDMA == 4 || G::NDMA == 2, "asm below is written for 2, 3, 4 or 6 pieces per wave");
    const uint64_t g0 = (uint64_t)(size_t)chunk + (uint64_t)wave * (G::NDMA * G::FRAG);       // wave-uniform
    const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)g0), hi32 = __builtin_amdgcn_readfirstlane((unsigned)(g0 >> 32));
    const uint64_t sbase = ((uint64_t)hi32 << 32) | lo32;
    const unsigned l0 = __builtin_amdgcn_readfirstlane(lds_off + (unsigned)wave * (G::NDMA * G::FRAG));
    unsigned keep;
    if constexpr (G::NDMA == 6) {
        // the instruction offset is added to the global AND to the LDS address; past its 4 KiB reach: a second lane
        // offset and M0 + 4096
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
                     "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %4, %2\n\t"
                     "global_load_lds_dwordx4 %4, %2 offset:1024\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(l0), "v"(voff + 4096u) : "memory", "scc");
    } else if constexpr (G::NDMA == 4) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(l0) : "memory");
    } else if constexpr (G::NDMA == 3) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(l0) : "memory");
    } else {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(l0) : "memory");
    }
}
template <int N>
__device__ __forceinline__ void dma_wait_b() {
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// fp16x3 column scale, plain columns: what a tail can make of accumulators bounded by amax_true — |q_l| <= w0 max_f |a_l|,
// |A_l| <= w0 max_f |Q_l|, |zbar_l| <= w0 max_f |hbar_l| + max_f |e_l| (`extra`; the quads' and jets' bounds: set_scale, dudf_sweep_bf16.hip)
__device__ __forceinline__ float plain_bound(float w0, float amax_true, float extra) { return w0 * amax_true + extra; }
// One product group: cc[u] += A[u] x B for TP tiles (rows of `af`: their pieces), chains interleaved, smallest terms first —
// fp16x3 (SP): lo*hi, hi*lo, hi*hi; bf16x6: mm, lh, hl, mh, hm, hh
template <int SP, int TP, int NPC>
__device__ __forceinline__ void mma_products(const u32x4 (*af)[NPC], const u32x4* bp, f32x4* cc) {
    constexpr int kA[6] = {1, SP ? 0 : 2, 0, 1, 0, 0}, kB[6] = {SP ? 0 : 1, SP ? 1 : 0, SP ? 0 : 2, 0, 1, 0};
#pragma unroll
    for (int i = 0; i < (SP ? 3 : 6); ++i)
#pragma unroll
        for (int u = 0; u < TP; ++u) {
            if constexpr (SP) cc[u] = mfma_h(as_h(af[u][kA[i]]), as_h(bp[kB[i]]), cc[u]);
            else cc[u] = mfma_b(as_bf(af[u][kA[i]]), as_bf(bp[kB[i]]), cc[u]);
        }
}
struct TailOps { f32x4 o1a, o2a, o3a, o1b, o2b, o3b, ba, bb; };   // operands of one pair of tiles (+ bias, forward sweeps)

// LDS offset of the per-layer running maxima: behind the three weight buffers — and behind the biases where the fp16x3 forward
// sweeps keep them (the quads' forward sweep has both)
template <int H, int SW, int SP>
__device__ __forceinline__ unsigned amax_lds_off(const SweepArgs& a) {
    return 3u * GeoB<H, SP>::CHUNKB + ((SP != 0 && base_of(SW) == SWEEP_FWD) ? (unsigned)(a.L * H * sizeof(float)) : 0u);
}

// Shared by the tile bodies, with the lane context of dudf_sweep_common.h.
__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
// fp16x3 column scale from a bound < 2^(E - 126) of the column: sb = 2^(15 - (E - 126)) brings it below 2^15, inv_sb = 1 / sb
__device__ __forceinline__ void col_scale(float bound, float& sb, float& inv_sb) {
    unsigned E = (__float_as_uint(bound) >> 23) & 255u;
    E = E < 27u ? 27u : (E > 250u ? 250u : E);             // all-zero (padding) columns, infinities: any finite scale will do
    sb = __uint_as_float((268u - E) << 23);
    inv_sb = __uint_as_float((E - 14u) << 23);
}
// max |.| over N accumulator tiles' registers and the 4 lane quarters: per column
template <int N>
__device__ __forceinline__ float col_absmax(const f32x4 (&t)[N]) {
    float m = 0.f;
    // dudf_track is inline asm, and these are MFMA results: hipcc's hazard recogniser does not see an asm statement's
    // register reads, so the wait states between the last MFMA and the first read are spelled out (found the hard way:
    // the last layer's column scale came from stale accumulators)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int T = 0; T < N; ++T) dudf_track(m, t[T]);
    m = fmaxf(m, __shfl_xor(m, 16));
    return fmaxf(m, __shfl_xor(m, 32));
}

// ---- output stage (fp32), shared by sweep_tile_b (forward sweeps) and sweep_tile_oct; sweep_tile_b's reverse sweep and sweep_tile_w
// keep copies, with the measured reason at each ----
// tile T's post-tail values `e` into the column's y partial sum (forward sweep) or df/dx accumulator (reverse sweep)
template <int BS, int H>
__device__ __forceinline__ void out_tile(const SweepArgs& a, int T, int li, int q, const f32x4 e, float& part, f32x4& accg) {
    if constexpr (BS == SWEEP_FWD) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(a.theta + a.off_wo + 16 * T + 4 * q);
        part += e[0] * wv[0] + e[1] * wv[1] + e[2] * wv[2] + e[3] * wv[3];
    } else if constexpr (BS == SWEEP_REV) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(a.w1t16 + li * H + 16 * T + 4 * q);
#pragma unroll
        for (int t = 0; t < 4; ++t) accg = mfma16(wv[t], e[t], accg);
    }
}
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }
// forward sweep, fixed-point stash: column p's scale in every layer (NaN: the column's output is not finite, see store_fx)
__device__ __forceinline__ void out_fxs(const SweepArgs& a, int64_t p, float sc) {
    for (int l = 0; l < a.L; ++l) a.fxs[(int64_t)l * a.np + p] = sc;
}
// reverse sweep: df/dx of column p (a poisoned column's cos came back as a finite number: NaN instead)
template <bool FX>
__device__ __forceinline__ void out_grad(const SweepArgs& a, int64_t p, f32x4 g, bool poison) {
    if constexpr (FX) { if (poison) g = f32x4{quiet_nan(), quiet_nan(), quiet_nan(), 0.f}; }
    *reinterpret_cast<f32x4*>(a.g + p * 4) = f32x4{g[0], g[1], g[2], 0.f};
}
// a wave that holds all of its columns' tiles (sweep_tile_b): the lane quarters' sums, b_out, y | df/dx
template <int BS, bool FX, bool CS>
__device__ __forceinline__ void out_finish(const SweepArgs& a, int64_t p, int q, bool isv, float part, const f32x4 accg, bool poison) {
    if constexpr (BS == SWEEP_FWD) {
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (isv) part += a.theta[a.off_bo];             // tangent / jet columns are derivatives: no constant term
        if (q == 0) a.y[p] = part;
        if constexpr (FX && CS) { if (q == 0 && nonfinite(part)) out_fxs(a, p, quiet_nan()); }
        else if constexpr (FX) { if (q == 0) out_fxs(a, p, nonfinite(part) ? quiet_nan() : 1.f); }   // plain columns: |sin| <= 1, the scale is 1
    } else if constexpr (BS == SWEEP_REV) {
        if (q == 0) out_grad<FX>(a, p, accg, poison);
    }
}

#if DUDF_FX_CHECK
// debug build only: ADDS this unit's copy of the counters the fixed-point packers bump (dudf_sweep_common.h) to out2 — [0] S/Q/A/Z, [1] C
int dudf_fx_read(unsigned* out2, int reset) {
    unsigned v[2];
    hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_dudf_fx_bad), sizeof(v));
    if (e == hipSuccess && reset) { const unsigned z[2] = {0u, 0u}; e = hipMemcpyToSymbol(HIP_SYMBOL(g_dudf_fx_bad), z, sizeof(z)); }
    if (e == hipSuccess) { out2[0] += v[0]; out2[1] += v[1]; }
    return (int)e;
}
#endif

}  // namespace
