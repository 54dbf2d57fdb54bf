// Which kernel instantiation a launch gets: ONE pure host function per kernel family (sweeps, pair launch, weight-gradient
// GEMM), the tables of the built (SW, FL) variants and the stash mask a workspace is promised.  No device code, no HIP header:
// everything here is a function of its arguments (the options come in as a value), so it is testable without a GPU
// (dudf_debug_kernel_choice, tests/test_kernel_choice.py).  The launchers in the .hip files only turn a choice into a launch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <utility>
#include "../../include/dudf_hip.h"

enum { SWEEP_FWD = 0, SWEEP_REV = 1, SWEEP_ADJ_FWD = 2, SWEEP_ADJ_REV = 3,
       SWEEP_FWD_H = 4, SWEEP_REV_H = 5, SWEEP_ADJ_FWD_H = 6, SWEEP_ADJ_REV_H = 7,     // Hessian-quad variants
       SWEEP_FWD_J = 8 };                                                              // third-order jets (query)

// ---- the run-time options, ONCE: X(name, lowest, highest, default of a fresh process).  dudf_set_option / dudf_get_option take the
// names; struct DudfOptions, the table of dudf_runtime.hip, the defaults and the current values all come from this list
#ifndef DUDF_STASH_DEFAULT
#define DUDF_STASH_DEFAULT 7          // requested stash mask of a fresh process: all seven arrays at 24 bits (R, E floats; C, S, Q, A, Z fixed point)
#endif
#ifndef DUDF_WGRAD_BUFFERS_DEFAULT
#define DUDF_WGRAD_BUFFERS_DEFAULT 4
#endif
#define DUDF_OPTION_LIST(X)                                                                                                            \
    X(deterministic, 0, 1, 0)              /* 1: every cross-workgroup sum of the training path — loss terms, loss_s2 statistics, dW, db — */ \
                                           /* has ONE owner (a single block for the loss sums, one column split per weight tile, one */ \
                                           /* block for the thin layers): bit-reproducible; slow (the weight-gradient GEMM runs on 7 CUs) */ \
    X(split, 0, 1, 1)                      /* operand split of the 16-bit matrix cores: 1 = fp16 hi/lo, three products, where it is */ \
                                           /* built; 0 = bf16x3, six, for every hidden matmul */                                       \
    X(split_quads, 0, 1, 1)                /* the Hessian quads / jets on fp16x3 as well (0: bf16x6) */                                \
    X(sweep_family, 0, 1, 1)               /* 1 = the 16-bit-core sweeps where built; 0 = the f32-input MFMA kernel everywhere (A/B reference) */ \
    X(stash, 0, 15, DUDF_STASH_DEFAULT)    /* REQUESTED stash mask, only 0, 6 or 7 (dudf_stash_mode reports what a workspace gets) */ \
    X(wgrad_family, 0, 2, 0)               /* weight-gradient GEMM: 0 = cooperative split (default), 1 = f32-input MFMA, 2 = bf16x6 per-wave split */ \
    X(wgrad_tr, 0, 1, 0)                   /* fp32 rows staged through the [column][feature] image + transposed fragment reads */      \
    X(pair_launch, 0, 1, 1)                /* quads + plain columns of a training sweep in ONE grid */                                 \
    X(wgrad_max_workgroups, 8, 256, 256)   /* cap of the weight-gradient GEMM's grid (256 = one workgroup per CU; a multi-GPU step leaves CUs to RCCL) */ \
    X(wgrad_buffers, 3, 4, DUDF_WGRAD_BUFFERS_DEFAULT)   /* LDS image buffers of the 24-bit-operand weight-gradient GEMM (4: one poll per stage instead of two) */

// snapshot of the run-time options (dudf_runtime.hip holds the current ones): the choosers read no globals.  A fresh one holds the defaults
struct DudfOptions {
#define X(name, lo, hi, def) int name = def;
    DUDF_OPTION_LIST(X)
#undef X
};
// which sweeps run fp16x3: bits 0-3 the plain columns' four sweeps (all or none: the adjoint reverse sweep's column scale
// comes from the fp16x3 adjoint forward sweep), bit 5 the Hessian quads / jets as well (option split_quads = 0: bf16x6)
inline int dudf_split_mask(const DudfOptions& o) { return o.split ? (15 | (o.split_quads ? 32 : 0)) : 0; }

// ---- the built variants: (SW, FL) pairs per family; p24 = the variant also has builds for a 24-bit stash -------------------
// FL: forward sweeps bit 0 = store h (S), bit 1 = store cos (C); reverse sweeps 1 = training stores; adjoint reverse 1 = e_l exists
struct DudfVariant { int sw, fl, p24; };
// dudf_sweep.hip: sweep_kernel<H, SW, FL>, H = 32 .. 512 (the forward tails always keep their outputs)
constexpr DudfVariant kF32Variants[] = {{0, 3, 0}, {1, 1, 0}, {1, 0, 0}, {2, 0, 0}, {3, 1, 0}, {3, 0, 0},
                                        {4, 1, 0}, {5, 1, 0}, {5, 0, 0}, {6, 0, 0}, {7, 0, 0}, {8, 0, 0}};
// dudf_sweep_bf16.hip, H = 128 | 256: sweep_bf16[_np]_kernel and sweep_f16[_np]_kernel<H, SW, FL>; p24 (H = 256 only):
// sweep_f16r[_np]_kernel (stash mask 6) and sweep_f16p[_np]_kernel (mask 7)
constexpr DudfVariant kSweepVariants[] = {{0, 3, 1}, {0, 2, 0}, {0, 0, 0}, {1, 1, 1}, {1, 0, 0}, {2, 0, 1}, {3, 1, 1}, {3, 0, 1},
                                          {4, 1, 1}, {4, 0, 0}, {5, 1, 1}, {5, 0, 0}, {6, 0, 1}, {7, 0, 1}, {8, 0, 0}};
// dudf_sweep_wide.hip, H = 512: sweep_w_kernel and sweep_w16_kernel<SW, FL>; p24: sweep_w16r_kernel (mask 6).  The stash array
// a layer's outputs travel through is written in every variant: the forward sweeps always store h_l
constexpr DudfVariant kWideVariants[] = {{0, 3, 1}, {0, 1, 0}, {1, 1, 1}, {1, 0, 0}, {2, 0, 1}, {3, 1, 1}, {3, 0, 1},
                                         {4, 1, 1}, {5, 1, 1}, {5, 0, 0}, {6, 0, 1}, {7, 0, 1}, {8, 0, 0}};
// pair launch (H = 256): sweep_pair_kernel<256, SW + 4, dudf_pair_flq(SW), SW, fl, SPQ, P24>, SPQ = 0 | 1 (quads on fp16x3),
// P24 = 0 | 6 | 7 (SPQ = 1 only): the training variants of the plain columns with the training variants of their quads
constexpr DudfVariant kPairVariants[] = {{0, 3, 1}, {1, 1, 1}, {2, 0, 1}, {3, 1, 1}};
constexpr int dudf_pair_flq(int sw) { return sw <= SWEEP_REV ? 1 : 0; }     // the quads' FL beside the plain columns' sweep sw
// run-time (sw, fl) -> the table entry as a compile-time constant: f(std::integral_constant<size_t, index>); the launchers
// instantiate exactly the kernels of the tables through this
template <size_t N, class F, size_t... I>
int dudf_with_variant(const DudfVariant (&t)[N], int sw, int fl, F&& f, std::index_sequence<I...>) {
    int rc = DUDF_E_UNSUPPORTED;
    (void)(((t[I].sw == sw && t[I].fl == fl) ? (rc = f(std::integral_constant<size_t, I>{}), true) : false) || ...);
    return rc;
}
template <size_t N, class F>
int dudf_with_variant(const DudfVariant (&t)[N], int sw, int fl, F&& f) { return dudf_with_variant(t, sw, fl, f, std::make_index_sequence<N>{}); }

// ---- LDS sizes (the .hip files assert them against their geometry structs) ---------------------------------------------------
constexpr int kMaxLdsBiasLayers = 32;      // fp16x3 forward sweeps: b_1..b_L live in LDS (32 KiB at H = 256); deeper nets: bf16x6
constexpr int kMaxAmaxLayers = 64;         // LDS words of the per-layer running maxima (deeper nets: no fp16x3 wgrad)
constexpr size_t kLdsCu = 160 * 1024;
constexpr size_t kAmaxBytes = kMaxAmaxLayers * sizeof(unsigned);
constexpr size_t kOctBytes = 8 * 2 * 1024 + 1024 + 8 * 64 * 16;      // B fragments | column maxima (2 x 128 floats) | output-stage partials
constexpr size_t dudf_chunk_bytes(int H, int pieces) { return (size_t)(H / 16) * pieces * 1024; }   // dudf_sweep16.h GeoB<H, SP>::CHUNKB
constexpr size_t dudf_wide_chunk_bytes(int pieces) { return (size_t)16 * pieces * 1024; }            // dudf_sweep_wide.hip GeoWT<SP>::CHUNKB
constexpr size_t dudf_bias_bytes(int L, int H) { return (size_t)L * H * sizeof(float); }

enum { DUDF_FAM_F32 = 0, DUDF_FAM_BF16, DUDF_FAM_F16, DUDF_FAM_F16R, DUDF_FAM_F16P,     // sweeps, H <= 256 (F32: every width)
       DUDF_FAM_W, DUDF_FAM_W16, DUDF_FAM_W16R,                                         // the 512-wide kernel: bf16x6, fp16x3, fp16x3 mask 6
       DUDF_FAM_PAIR,
       DUDF_FAM_WG_F32, DUDF_FAM_WG_BF16, DUDF_FAM_WG_BF16P, DUDF_FAM_WG_F16P, DUDF_FAM_WG_F16TR, DUDF_FAM_WG_F16P24 };

struct SweepRequest {
    int which, H, L;
    int store_s, store_c, train, have_e;   // what the sweep has to leave behind / whether SWEEP_ADJ_FWD produced e_l
    int split, p24;                        // dudf_split_mask, the workspace's stash mask
    bool ebound, zbound;                   // the workspace has these side arrays
};
struct SweepChoice {
    int status;            // 0 | DUDF_E_UNSUPPORTED | DUDF_E_BADMODE
    int family, H;         // H: the kernel's width parameter (weight gradients of 512-wide layers: 2 x 2 tiles of the 256 build)
    int sw, fl;            // the instantiation (pair launch: the plain columns' part; weight gradients: fl = VAR or 0)
    int swq, flq, spq;     // pair launch: the quads' part, and whether it is fp16x3
    int p24;               // stash mask the kernel is built for
    int no_pk;             // the build without packed fp32 instructions
    int products;          // per algorithmic multiply: 1 f32-input MFMA, 3 fp16 hi/lo split, 6 three-piece bf16 split
    size_t lds, lds_max;   // dynamic LDS bytes of the launch / what is set once as the function's maximum
    int store_s, store_c;  // the stash flags the kernel is launched with (the f32 family's forward tails always store)
    int remap;             // weight gradients: the 2 x 2 tiles of a group remapped onto one XCD (1-D grid)
};
inline SweepChoice dudf_no_choice(int status) { SweepChoice c = {}; c.status = status; return c; }
template <int SW> constexpr bool sweep_no_pk() { return SW == SWEEP_FWD || SW >= SWEEP_FWD_H; }

namespace dudf_detail {
inline SweepChoice sweep_choice(const SweepRequest& r, int family, int sw, int fl, int products, size_t lds, size_t lds_max) {
    SweepChoice c = {};
    c.family = family; c.H = r.H; c.sw = sw; c.fl = fl; c.products = products; c.lds = lds; c.lds_max = lds_max;
    c.p24 = family == DUDF_FAM_F16P ? 7 : (family == DUDF_FAM_F16R || family == DUDF_FAM_W16R) ? 6 : 0;
    c.no_pk = (family >= DUDF_FAM_BF16 && family <= DUDF_FAM_F16P) && (sw == SWEEP_FWD || sw >= SWEEP_FWD_H);
    c.store_s = r.store_s; c.store_c = r.store_c;
    return c;
}
// the flags -> FL of a sweep where every variant is built (bf16x6 / fp16x3 at 128 | 256); -1: no such variant
inline int fl_of(const SweepRequest& r) {
    switch (r.which) {
        case SWEEP_FWD: return (r.store_s && r.store_c) ? 3 : r.store_c ? 2 : !r.store_s ? 0 : -1;   // value+gradient query: only cos is read again
        case SWEEP_REV: case SWEEP_REV_H: return r.train ? 1 : 0;
        case SWEEP_ADJ_REV: return r.have_e ? 1 : 0;
        case SWEEP_FWD_H: return r.store_s ? 1 : 0;                                                 // queries do not need h | hdot again
        default: return 0;
    }
}
// H = 128 | 256: fp16x3 where the split mask, the side arrays and the depth allow it, bf16x6 otherwise; a 24-bit workspace (H = 256)
// has only the fp16x3 training variants built for its mask
inline SweepChoice choose_b(const SweepRequest& r) {
    const int which = r.which, H = r.H;
    const size_t w3 = 3 * dudf_chunk_bytes(H, 2);
    // fp16x3 with stash mask 0 / 6 / 7: its own build each (training variants only; a 24-bit workspace holds C as fixed point)
    auto f16 = [&](int fl, size_t lds, bool train_variant) {
        if (r.p24 && !train_variant) return dudf_no_choice(DUDF_E_UNSUPPORTED);
        int fam = DUDF_FAM_F16;
        if (r.p24) {
            if (H == 256 && r.p24 == 7) fam = DUDF_FAM_F16P;
            else if (H == 256 && r.p24 == 6) fam = DUDF_FAM_F16R;
            else return dudf_no_choice(DUDF_E_UNSUPPORTED);
        }
        return sweep_choice(r, fam, which, fl, 3, lds, kLdsCu);
    };
    if (which <= SWEEP_ADJ_REV && ((r.split >> which) & 1)) {                 // the plain columns' four sweeps
        const size_t oct = H == 256 ? kOctBytes : 0;                         // + the exchange area of the one-group pass
        const size_t lds_f = w3 + dudf_bias_bytes(r.L, H) + oct;             // + the biases (forward sweep)
        const size_t lds_o = w3 + kAmaxBytes + oct;                          // + the per-layer running maxima
        if (which == SWEEP_FWD && r.L <= kMaxLdsBiasLayers) {
            const int fl = fl_of(r);
            return fl < 0 ? dudf_no_choice(r.p24 ? DUDF_E_UNSUPPORTED : DUDF_E_BADMODE) : f16(fl, lds_f, fl == 3);
        }
        if (which == SWEEP_REV) return f16(r.train ? 1 : 0, lds_o, r.train);
        if (which == SWEEP_ADJ_FWD) return f16(0, lds_o, true);
        if (which == SWEEP_ADJ_REV && (!r.have_e || (r.ebound && ((r.split >> SWEEP_ADJ_FWD) & 1)))) return f16(r.have_e ? 1 : 0, lds_o, true);
        if (r.p24) return dudf_no_choice(DUDF_E_UNSUPPORTED);                 // a 24-bit workspace has no other kernels
    }
    // ... and the Hessian quads' sweeps (split mask bit 5; option split_quads).  All of a workspace's or none: the forward sweep
    // leaves zbound for the other three, the adjoint forward sweep ebound for the adjoint reverse one.
    if (which >= SWEEP_FWD_H && which <= SWEEP_ADJ_REV_H && (r.split & 32) && r.zbound && r.L <= kMaxLdsBiasLayers) {
        const size_t lds_q = w3 + kAmaxBytes, lds_fq = lds_q + dudf_bias_bytes(r.L, H);
        if (which == SWEEP_FWD_H) return f16(r.store_s ? 1 : 0, lds_fq, r.store_s);
        if (which == SWEEP_REV_H) return f16(r.train ? 1 : 0, lds_q, r.train);
        if (r.ebound) return f16(0, lds_q, true);
    }
    if (r.p24 && which != SWEEP_FWD_J) return dudf_no_choice(DUDF_E_UNSUPPORTED);     // (the jets stash nothing)
    if (which == SWEEP_FWD_J && (r.split & 32) && r.L <= kMaxLdsBiasLayers)            // third-order jets (curvature query)
        return sweep_choice(r, DUDF_FAM_F16, which, 0, 3, w3 + kAmaxBytes + dudf_bias_bytes(r.L, H), kLdsCu);
    const int fl = fl_of(r);
    if (fl < 0) return dudf_no_choice(DUDF_E_BADMODE);
    const size_t lds = 3 * dudf_chunk_bytes(H, 3) + kAmaxBytes;
    return sweep_choice(r, DUDF_FAM_BF16, which, fl, 6, lds, lds);
}
// H = 512: fp16x3 or bf16x6 by the split mask (plain columns by their bit, quads and jets by bit 5)
inline SweepChoice choose_w(const SweepRequest& r) {
    const int which = r.which;
    const bool h16 = which <= SWEEP_ADJ_REV ? ((r.split >> which) & 1) != 0 : (r.split & 32) != 0;
    int fl = fl_of(r);
    if (which == SWEEP_FWD) fl = r.store_c ? 3 : 1;
    if (which == SWEEP_FWD_H) fl = 1;
    const size_t lds16 = 3 * dudf_wide_chunk_bytes(2) + kAmaxBytes, lds = 3 * dudf_wide_chunk_bytes(3) + kAmaxBytes;
    if (r.p24) {                                     // a training workspace with R, E, C at 24 bits: its training variants only
        const bool train_variant = which == SWEEP_FWD ? (r.store_s && r.store_c) : which == SWEEP_FWD_H ? r.store_s != 0
                                 : (which == SWEEP_REV || which == SWEEP_REV_H) ? r.train != 0 : which != SWEEP_FWD_J;
        if (r.p24 != 6 || !h16 || !train_variant) return dudf_no_choice(DUDF_E_UNSUPPORTED);
        return sweep_choice(r, DUDF_FAM_W16R, which, fl, 3, lds16, lds16);
    }
    return h16 ? sweep_choice(r, DUDF_FAM_W16, which, fl, 3, lds16, lds16) : sweep_choice(r, DUDF_FAM_W, which, fl, 6, lds, lds);
}
}  // namespace dudf_detail

inline bool dudf_sweep_bf16_supported(int which, int H, int L) {
    return (H == 512 || H == 256 || H == 128) && L >= 2 && which >= SWEEP_FWD && which <= SWEEP_FWD_J;
}

// One column range of one sweep.  The 16-bit-core families where they are built (option sweep_family); the plain columns fall
// through to the f32-input kernel when those have no kernel for the request (a 24-bit workspace has no other: an error).
inline SweepChoice dudf_choose_sweep(SweepRequest r, const DudfOptions& o) {
    if (r.which < SWEEP_FWD || r.which > SWEEP_FWD_J) return dudf_no_choice(DUDF_E_BADMODE);
    if (o.sweep_family && dudf_sweep_bf16_supported(r.which, r.H, r.L)) {
        const SweepChoice c = r.H == 512 ? dudf_detail::choose_w(r) : dudf_detail::choose_b(r);
        if (r.which >= SWEEP_FWD_H || c.status != DUDF_E_UNSUPPORTED) return c;
    }
    if (r.which <= SWEEP_ADJ_REV && r.p24) return dudf_no_choice(DUDF_E_UNSUPPORTED);
    if (r.which == SWEEP_FWD) r.store_s = r.store_c = 1;      // the f32 kernel only builds its stash-everything variant: the
    if (r.which == SWEEP_FWD_H) r.store_s = 1;                // leaner ones made the register allocator spill
    if (!(r.H == 32 || r.H == 64 || r.H == 128 || r.H == 256 || r.H == 512)) return dudf_no_choice(DUDF_E_BADCFG);
    const int fl = r.which == SWEEP_FWD ? 3 : dudf_detail::fl_of(r);
    const size_t lds = 2 * 32 * (size_t)(r.H + 4) * sizeof(float);           // two chunk buffers of 32 padded rows
    return dudf_detail::sweep_choice(r, DUDF_FAM_F32, r.which, fl, 1, lds, lds);
}

// Quads (variant base + 4) and plain columns (variant base, fp16x3) of a training sweep at H = 256 in ONE grid;
// DUDF_E_UNSUPPORTED when the combination has no pair kernel (the caller then launches them one after the other).
// `r`: the plain columns' request (both ranges share their flags).
inline SweepChoice dudf_choose_pair(const SweepRequest& r, const DudfOptions& o) {
    const int base = r.which;
    const SweepChoice no = dudf_no_choice(DUDF_E_UNSUPPORTED);
    if (!o.sweep_family || !o.pair_launch || r.H != 256 || base < SWEEP_FWD || base > SWEEP_ADJ_REV) return no;
    if (!((r.split >> base) & 1) || r.L < 2 || r.L > kMaxLdsBiasLayers) return no;
    // the training variants only (a query has no plain columns beside its quads)
    if (base == SWEEP_FWD && !(r.store_s && r.store_c)) return no;
    if (base == SWEEP_REV && !r.train) return no;
    if (base == SWEEP_ADJ_REV && !(r.have_e && r.ebound && ((r.split >> SWEEP_ADJ_FWD) & 1))) return no;
    const size_t w3 = 3 * dudf_chunk_bytes(256, 2), bias = base == SWEEP_FWD ? dudf_bias_bytes(r.L, 256) : 0;
    const size_t lds_p = w3 + (base == SWEEP_FWD ? bias : kAmaxBytes) + kOctBytes;
    const bool q16 = (r.split & 32) && r.zbound && r.ebound;       // the quads on fp16x3 as well (their LDS is then the smaller part)
    const size_t lds_q = q16 ? w3 + bias + kAmaxBytes : 3 * dudf_chunk_bytes(256, 3) + kAmaxBytes;
    if (r.p24 && !(q16 && (r.p24 == 6 || r.p24 == 7))) return no;  // (the 24-bit stash needs the quads on fp16x3 too: dudf_stash_p24_enabled)
    SweepChoice c = dudf_detail::sweep_choice(r, DUDF_FAM_PAIR, base, base == SWEEP_ADJ_FWD ? 0 : base == SWEEP_FWD ? 3 : 1, 3,
                                              lds_q > lds_p ? lds_q : lds_p, kLdsCu);      // the plain columns of a pair launch are always fp16x3
    c.swq = base + 4; c.flq = dudf_pair_flq(base); c.spq = q16; c.p24 = r.p24; c.no_pk = 1;
    return c;
}

// The hidden layers' weight-gradient GEMM.  H, L: the network; p24: bit 0 of the stash mask (24-bit operands); np: the column stride.
struct WgradRequest { int H, L, p24; int64_t np; };
inline SweepChoice dudf_choose_wgrad(const WgradRequest& r, const DudfOptions& o) {
    const int H = r.H == 512 ? 256 : r.H, ntz = (r.H / H) * (r.H / H);     // 512: 2 x 2 output tiles of 256 x 256
    auto pick = [&](int family, int var, int products, size_t lds) {
        SweepChoice c = {};
        c.family = family; c.H = H; c.fl = var; c.products = products; c.lds = c.lds_max = lds; c.p24 = family == DUDF_FAM_WG_F16P24;
        c.no_pk = family >= DUDF_FAM_WG_BF16P;
        return c;
    };
    if (!(H == 32 || H == 64 || H == 128 || H == 256)) return dudf_no_choice(DUDF_E_BADCFG);
    // 24-bit operands: only the cooperative-split fp16x3 kernel reads them
    if (r.p24 && (o.wgrad_family != 0 || H != 256)) return dudf_no_choice(DUDF_E_UNSUPPORTED);
    if (o.wgrad_family == 1) return pick(DUDF_FAM_WG_F32, 0, 1, 4 * (size_t)(H / 4) * 33 * 4 * sizeof(float));   // 2 buffers x (X tile + Y tile), rows padded to 33
    const size_t lds_wave = (size_t)4 * 2 * (H / 4) * 16 * 4 * sizeof(float);                                  // ring of 4 x (X image + Y image)
    // per-wave split: narrow layers, option wgrad_family = 2, and beyond the 32-bit lane byte offsets of the cooperative kernel's staging loads
    if (H != 256 || o.wgrad_family == 2 || (int64_t)(r.H / 4) * r.np * 16 >= (1ll << 32)) return pick(DUDF_FAM_WG_BF16, 0, 6, lds_wave);
    // The cooperative-split body (conflict-free producer lanes, progress flags in LDS instead of a stage barrier, MFMAs first, split
    // two images ahead, SIMD partners alternating on the matrix pipe) has two builds, named by `var`: 9 = three image buffers,
    // 25 = four; DESIGN.md Appendix A has the numbers of its predecessors.  fp16x3 needs the running maxima of every layer in LDS (L <= 64).
    const bool f16 = o.split && r.L <= kMaxAmaxLayers;
    const size_t lds_t = (size_t)(2 * 2 * 16 * 576);            // one buffer: (X | Y) x 2 pieces x 16 rows of 576 B; + 512: the flags
    if (r.p24) {                                                // 24-bit tile-major operands: their own build, three or four buffers
        if (!(f16 && ntz == 1)) return dudf_no_choice(DUDF_E_UNSUPPORTED);
        return o.wgrad_buffers == 4 ? pick(DUDF_FAM_WG_F16P24, 25, 3, 4 * lds_t + 512) : pick(DUDF_FAM_WG_F16P24, 9, 3, 3 * lds_t + 512);
    }
    if (o.wgrad_tr && f16 && ntz == 1 && !o.deterministic) return pick(DUDF_FAM_WG_F16TR, 9, 3, 3 * lds_t + 512);
    const size_t lds_piece = (size_t)2 * (H / 32) * 2 * (32 * 16 + 16);      // one buffer: (X | Y) x blocks, per piece
    if (f16) {
        // (three image buffers: the four-buffer form of the body, var 25, is 2-3 % SLOWER with fp32 operands — 0.557 vs 0.543 ms
        //  at 256, 2.52 vs 2.46 ms at 512, profiles/r05_j_ab512.txt — and 2-3 % faster with 24-bit ones)
        SweepChoice c = pick(DUDF_FAM_WG_F16P, 9, 3, 3 * 2 * lds_piece + 512);
        c.remap = ntz == 4 && !o.deterministic;                 // 2 x 2 tiles: a group's tiles on one XCD
        return c;
    }
    return pick(DUDF_FAM_WG_BF16P, 9, 6, 3 * 3 * lds_piece + 512);          // bf16x6 (option split = 0), same body
}

// Option "stash" (format of the stash a training workspace keeps; dudf_stash_mode returns what a given workspace gets):
//   0  = every array fp32, 17 array-layer units per column (rounds 1-3);
//   6  = R and E as 24-bit floats, C as 24-bit fixed point, tile-major (dudf_internal.h): 15 units.  Every tolerance
//        holds, the 12-step beetle trajectory included (3e-7 .. 5e-7, as with fp32);
//   7  = S, Q, A, Z as 24-bit FIXED POINT relative to a per-column power of two as well (12.75 units; the default): every
//        single-step tolerance and every trajectory bar holds (round 4 stored these four as 24-bit FLOATS: 2^-17 noise on the
//        weight-gradient GEMM's operands moved the beetle trajectory by 4e-4, bar 1e-4; tests/test_stash_p24_gpu.py).
// The 24-bit arrays exist in the fp16x3 training kernels of 256- and 512-wide networks and in the cooperative-split weight-gradient
// GEMM; an option that routes a kernel elsewhere drops the corresponding bits.  Every mask promised here must have a kernel for
// every sweep of a step and for the GEMM: tests/test_kernel_choice.py walks the option space.
inline int dudf_stash_p24_enabled(int H, int L, const DudfOptions& o) {
    int want = o.stash & 7;
    if (want != 0 && want != 6 && want != 7) want = 6;
    if (!(o.sweep_family && o.split && (dudf_split_mask(o) & 47) == 47)) want = 0;
    if (o.wgrad_family != 0) want &= 6;       // f32 / per-wave weight-gradient kernels read fp32 rows
    if (H == 256 && L >= 2 && L <= 32) return want;
    // the 512-wide kernel relays S, Q, A, Z through the stash as fp32; R, E, C are not relays.  (Round 5 built the relay as the
    // fixed-point array — every single-step tolerance held, the 12-step trajectory did not: 6e-4 against 7e-7, the rounding enters
    // the layer chain itself there, not only the weight-gradient GEMM's operands — tests/test_traj512_gpu.py)
    if (H == 512 && L >= 2) return want & 6;
    return 0;
}

// the kernel's name as a profiler prints it (without namespace and argument list), e.g. sweep_f16p_np_kernel<256,0,3>
inline int dudf_choice_name(const SweepChoice& c, char* buf, size_t n) {
    const char* np = c.no_pk ? "_np" : "";
    switch (c.family) {
        case DUDF_FAM_F32: return snprintf(buf, n, "sweep_kernel<%d,%d,%d>", c.H, c.sw, c.fl);
        case DUDF_FAM_BF16: return snprintf(buf, n, "sweep_bf16%s_kernel<%d,%d,%d>", np, c.H, c.sw, c.fl);
        case DUDF_FAM_F16:
            return snprintf(buf, n, "sweep_f16%s_kernel<%d,%d,%d>", np, c.H, c.sw, c.fl);
        case DUDF_FAM_F16R: return snprintf(buf, n, "sweep_f16r%s_kernel<%d,%d,%d>", np, c.H, c.sw, c.fl);
        case DUDF_FAM_F16P: return snprintf(buf, n, "sweep_f16p%s_kernel<%d,%d,%d>", np, c.H, c.sw, c.fl);
        case DUDF_FAM_W: return snprintf(buf, n, "sweep_w_kernel<%d,%d>", c.sw, c.fl);
        case DUDF_FAM_W16: return snprintf(buf, n, "sweep_w16_kernel<%d,%d>", c.sw, c.fl);
        case DUDF_FAM_W16R: return snprintf(buf, n, "sweep_w16r_kernel<%d,%d>", c.sw, c.fl);
        case DUDF_FAM_PAIR: return snprintf(buf, n, "sweep_pair_kernel<256,%d,%d,%d,%d,%d,%d>", c.swq, c.flq, c.sw, c.fl, c.spq, c.p24);
        case DUDF_FAM_WG_F32: return snprintf(buf, n, "wgrad_hidden_kernel<%d>", c.H);
        case DUDF_FAM_WG_BF16: return snprintf(buf, n, "wgrad_hidden_bf16_kernel<%d>", c.H);
        case DUDF_FAM_WG_BF16P: return snprintf(buf, n, "wgrad_hidden_bf16p_kernel<%d,%d>", c.H, c.fl);
        case DUDF_FAM_WG_F16P: return snprintf(buf, n, "wgrad_hidden_f16p_kernel<%d,%d>", c.H, c.fl);
        case DUDF_FAM_WG_F16TR: return snprintf(buf, n, "wgrad_hidden_f16tr_kernel<%d,%d>", c.H, c.fl);
        case DUDF_FAM_WG_F16P24: return snprintf(buf, n, "wgrad_hidden_f16p24_kernel<%d,%d>", c.H, c.fl);
        default: return snprintf(buf, n, "?");
    }
}
