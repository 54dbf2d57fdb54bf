// The SIREN sweeps (plain columns, Hessian quads, third-order jets; 256- and 128-wide layers) on the bf16 matrix cores at
// fp32 accuracy ("bf16x6", gfx950 / CDNA4).
//
// Same sweeps, same tails, same stash as dudf_sweep.hip (see there for what each sweep computes and which reference
// lines it replaces); what changes is how a hidden layer  OUT[feature][column] = M[feature][k] * IN[k][column]  is
// multiplied: on v_mfma_f32_16x16x32_bf16 with every fp32 operand split exactly into three bf16 pieces, or on the fp16
// instruction with two (dudf_sweep16.h: the split, the weight image and the helpers built on them).
//
// The 16-bit sweeps are three translation units over that header.  This one holds the scheme for 128- and 256-wide layers — a
// layer's accumulators stay in registers (sweep_tile_b, sweep_tile_oct), the kernels of its four families, the pair kernel and
// their launchers — and dudf_launch_sweep_bf16, which sends 512-wide layers on to dudf_sweep_wide.hip: there a layer's outputs
// reach the next one through the stash (sweep_tile_w).  dudf_prep.hip holds the kernels that write what both read: the weight
// images (pack_bf16_kernel, pack_f16_kernel) and the one launch in front of a training forward (prep_kernel).
//
// Mapping (output-stationary, K streamed):
//   * a wave owns 16 columns for a whole sweep; a workgroup is 8 waves = 128 columns, two waves per SIMD, one
//     workgroup per CU.  The accumulator tile of v_mfma_f32_16x16x32_bf16 has the layout of the f32 instruction
//     (row = 4*(lane>>4)+reg = feature, col = lane&15 = column), so all tails are shared (dudf_sweep_common.h) and the
//     stash layout is unchanged.
//   * a layer keeps ALL its 16 output tiles in accumulators (64 registers) and streams over the 8 k-blocks of 32
//     input features.  The B operand of k-block kb wants, per lane, 8 k of one column (k = 8*(lane>>4) + e).  K is a
//     contraction index, so a permutation applied to both operands is free: k-slot (g, e) is mapped to feature
//     32kb + 4g + e (e < 4) or 32kb + 16 + 4g + (e-4) — exactly the 4+4 accumulator registers a lane holds of tiles
//     2kb and 2kb+1 of the PREVIOUS layer.  So step kb runs the elementwise tail (bias, sin/cos or the adjoint
//     formulas, stash stores) of those two tiles of the previous layer, splits the 8 results into pieces and packs
//     them (v_cvt_pk_bf16_f32) into 12 registers: the B operand, used at once by 16 tiles x 6 MFMAs and then dead.
//     Activations never touch LDS, and the tail of step kb+1 overlaps the MFMAs of step kb inside a wave.
//   * the weights are pre-split once per step (dudf_prep.hip) into an image in A-FRAGMENT ORDER (dudf_sweep16.h): the 48 KiB
//     of a k-block (16 tiles x 3 pieces at H = 256) are contiguous and go to LDS verbatim.  Three buffers (144 KiB), fetched
//     two steps ahead, one barrier per
//     k-block, hand-counted vmcnt as in the f32 kernel.  128 columns share every byte fetched from L2: at bf16 rates
//     the f32 kernel's 64-column workgroups would be bound by L2 -> LDS weight traffic, not by the matrix cores.
//   * the first layer (K = 3+1) and the output / df/dx matmuls stay on the fp32 MFMA.
#include "dudf_sweep16.h"

// Variants that were built, measured and NOT kept (tails of a pair half a step apart, one operand set for the fp16x3 adjoint
// forward sweep, one tile at a time, DMA pieces issued by the idle half of a partial pass, static / per-phase wave priorities,
// other fragment prefetch distances and feed / tail slots) are no longer in this file: DESIGN.md Appendix A has their numbers,
// `git log -- diffudf_amd/csrc/dudf_sweep_bf16.hip` (round 3) their code.

namespace {

// One pass: the workgroup's waves 0..nact-1 take the 16-column groups g_first.. through a whole sweep.  Waves beyond
// nact (the last, partial pass of a workgroup's share) only keep the weight stream and the barriers going.
template <int H, int SW, int FL, int SP = 0, int P24 = 0>
__device__ __forceinline__ void sweep_tile_b(const SweepArgs& a, const int g_first, const int nact, char* lds, unsigned& gc) {
    using G = GeoB<H, SP>;
    constexpr int NPC = G::NPC;
    static_assert(SP == 0 || SW <= SWEEP_FWD_J, "fp16x3: plain columns, Hessian quads, jets");
    static_assert(P24 == 0 || ((P24 == 6 || P24 == 7) && SP != 0 && H == 256 && !is_jet(SW)), "24-bit stash arrays (mask 6: R, E, C; 7: S, Q, A, Z as well): the fp16x3 training kernels of 256-wide layers");
    constexpr int BS = base_of(SW);
    constexpr bool HS = is_hess(SW);                   // quads: lane & 3 = channel (0 = value, 1 + k = tangent d/dx_k); jets:
                                                       // lane & 15 = Taylor monomial (0 = value), see dudf_sweep_common.h
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, q = lane >> 4;
    const bool isv = !HS || (is_jet(SW) ? li == 0 : (lane & 3) == 0);   // value channel (always, on the plain path)
    const int nhid = a.L - 1;                          // hidden x hidden layers (>= 1 here)
    constexpr bool kFwdDir = fwd_dir<SW>();

    f32x4 acc[G::NT], prev[G::NT];                     // this layer's accumulators / the previous layer's, tails pending
    const int64_t p = (int64_t)(g_first + wave) * 16 + li;
    auto image = [&](int j) -> const char* { return sweep_image<SW, G::IMGB, SP>(a, nhid, j); };
    // fp16x3: the accumulators of matrix j hold 2^k_j (W h); `unscale` = 2^-k_j of the matrix whose outputs wait in `prev`
    // (1 for the first layer, which runs on the fp32 MFMA) — folded into the bias add of the forward tail
    float unscale = 1.f;
    auto unscale_of = [&](int j) -> float { return sweep_unscale<SW>(a, nhid, j); };
    // fp16x3, B operand.  The forward sweep's is h_l = sin(.): |h| <= 1 fits fp16 as it stands (small values keep an absolute
    // error of 2^-25: fp16 subnormals are honoured).  The other sweeps' operands (q_l, A_l, zbar_l) have no a-priori size, so
    // every COLUMN gets its own power of two `sb`, fixed when the previous layer's accumulators are final — before any of
    // its tails has run — from a bound: |q_l| <= w0 max_f |a_l|, |A_l| <= w0 max_f |Q_l|, |zbar_l| <= w0 max_f |hbar_l| +
    // max_f |e_l| (the last term left per layer and column by the adjoint forward sweep, SweepArgs::ebound).  The scaled
    // column stays below 2^15; a bound that is loose by 2^m costs m of the 16 bits by which fp16's subnormal floor sits
    // below fp32's half ulp of the column maximum.  `unscale` (per lane = per column) turns the accumulators of the matrix
    // that consumed the scaled operand back into true values: 2^-k_j / sb.
    // Hessian quads: the forward sweep's tangent channels hdot^k = w0 c zdot^k are not bounded by 1 either, and the other
    // sweeps' tails couple the four channels of a quad — their bounds (set_scale) take two more per-column maxima: max_f
    // |zdot_l| of the tangent columns, left per layer by the quads' forward sweep (SweepArgs::zbound), and max_f |e_l|.
    constexpr bool kColScale = SP != 0 && (BS != SWEEP_FWD || HS);
    constexpr bool kTrackE = SP != 0 && BS == SWEEP_ADJ_FWD;   // (the fp16x3 adjoint reverse sweep therefore needs the fp16x3 adjoint forward one)
    float sb = 1.f, inv_sb = 1.f;                       // scale of the B operand being built (tails of `prev`) and its inverse
    // amax_true: max_f |accumulator| of this column (true values); extra: the bound of what the tail adds (adjoint reverse:
    // e_l); zb: max_f |zdot_l| of this column (quads, tangent channels).  Quads (tails in dudf_sweep_common.h::epilogue):
    //   forward          value: |sin| <= 1                  tangent k: w0 |zdot^k|
    //   reverse          value: w0 |a|                       tangent k: w0 (|adot^k| + w0 |zdot^k| |a|)           (a of the value channel)
    //   adjoint forward  value: w0 (|Q| + w0 sum_k |zdot^k| |Qdot^k|)                tangent k: w0 |Qdot^k|
    //   adjoint reverse  value: |E| + w0 |hbar| + w0^2 sum_k |zdot^k| |hdotbar^k|   tangent k: |E| + w0 |hdotbar^k|
    auto set_scale = [&](float amax_true, float extra, float zb) {
        float bound;
        if constexpr (!HS) { (void)zb; bound = plain_bound(a.w0, amax_true, extra); }
        else if constexpr (is_jet(SW)) {
            // (a second copy of the polynomial of epilogue<SWEEP_FWD_J>, dudf_sweep_common.h — keep the two in step: as ONE function all
            //  11 jet kernels of the three units changed and 6 of them spill more, up to 1920 bytes of scratch from none: outside the
            //  per-kernel limit "scratch not larger", tools/asm_diff.py)
            // third-order jets: the tail of a monomial's column multiplies lower-order columns of the same point (epilogue,
            // SWEEP_FWD_J) — the same combination, evaluated on the columns' maxima, bounds it (|sin|, |cos| <= 1)
            const int l0 = lane & 48;
            const unsigned jw = kJetLane[lane & 15];
            const float w2 = 0.5f * (float)((jw >> 24) & 3), w3 = 0.5f * (float)((jw >> 26) & 3);
            const float F[3] = {a.w0 * __shfl(amax_true, l0 + 1), a.w0 * __shfl(amax_true, l0 + 2), a.w0 * __shfl(amax_true, l0 + 3)};
            auto sel = [&](unsigned k) -> float { k &= 3; return k == 0 ? F[0] : (k == 1 ? F[1] : F[2]); };
            const float S0 = a.w0 * __shfl(amax_true, l0 + (int)(jw & 15)), S1 = a.w0 * __shfl(amax_true, l0 + (int)((jw >> 4) & 15)),
                        S2 = a.w0 * __shfl(amax_true, l0 + (int)((jw >> 8) & 15));
            const float fab = sel(jw >> 18) * sel(jw >> 20);
            const float p2 = S0 * sel(jw >> 12) + S1 * sel(jw >> 14) + S2 * sel(jw >> 16) + w2 * fab;
            const float p3 = w3 * fab * sel(jw >> 22);
            bound = ((jw >> 28) & 1) ? 1.f : a.w0 * amax_true + p3 + p2;
        }
        else if constexpr (BS == SWEEP_FWD) bound = isv ? 1.f : a.w0 * amax_true;
        else if constexpr (BS == SWEEP_REV) {
            const float av = quad_bcast0(amax_true);
            bound = a.w0 * (amax_true + (isv ? 0.f : a.w0 * zb * av));
        } else {
            const float sk = quad_sum(isv ? 0.f : zb * amax_true);
            bound = extra + a.w0 * (amax_true + (isv ? a.w0 * sk : 0.f));
        }
        // 2^-10 of head room: the bound is formed in rounded fp32 and from the UNROUNDED e_l / zdot_l maxima, while the tails round
        // on their own path (and R, E come back rounded to 16 significant bits): a column whose bound sits an ulp under a power of two
        // could hand the fixed-point stash a value a grid step outside [-1, 1] 2^E, which fx24_pack would wrap to +5 2^E.
        // Once per layer and column, not per value; costs a bit of the column's precision in 0.14 % of the scale decisions.
        col_scale(bound * DUDF_FX_HEADROOM, sb, inv_sb);
    };
    auto ebound_of = [&](int layer) -> float {                 // adjoint reverse sweep with df/dx terms: max_f |e_layer| of this column
        if constexpr (kColScale && BS == SWEEP_ADJ_REV && (HS || (FL & 1) != 0)) return a.ebound[(int64_t)layer * a.np + p];
        return 0.f;
    };
    auto zbound_of = [&](int layer) -> float {                 // quads behind the forward sweep: max_f |zdot_layer| of this column
        if constexpr (kColScale && HS && BS != SWEEP_FWD) return a.zbound[(int64_t)layer * a.nch + p];
        return 0.f;
    };
    auto store_zbound = [&](int layer, float m) {              // the quads' forward sweep leaves it (0 in the value columns)
        if constexpr (kColScale && HS && !is_jet(SW) && BS == SWEEP_FWD) a.zbound[(int64_t)layer * a.nch + p] = isv ? 0.f : m;   // (every lane, no branch: see store_fx)
    };
    float eb_next = 0.f, zb_next = 0.f;
    // running max |.| of what this sweep's tails store for the weight-gradient GEMM (q_l, A_l or zbar_l), per layer: lanes
    // -> one LDS word per layer (ds_max_u32 on the bit patterns: non-negative floats order like integers) -> HBM at kernel end
    constexpr int kRow = amax_row<SW, FL>();
    constexpr bool kFx = (P24 & 1) != 0;                // S, Q, A, Z as 24-bit fixed point relative to the column's bound (dudf_sweep_common.h)
    TailTrackT<kFx> tmax;
    // the power of two the readers of this sweep's fixed-point array multiply with, per layer and column (SweepArgs::fxs): 2^E of
    // set_scale, or 1 where no column scale exists (plain forward sweep: |sin| <= 1)
    // A fixed-point value cannot be a NaN or an infinity (their bit patterns decode to finite numbers), so the COLUMN SCALE carries
    // them: a column whose inputs are not finite — the network's output y (reverse sweep; the forward sweep checks its own y at
    // the end of the pass), the loss cotangents ybar / gbar (adjoint sweeps: a wrong `n_on_surface` hint arrives as NaN cotangents)
    // — stores NaN as its 2^E, and every reader's (t - 3) 2^E is NaN: d(theta) of a poisoned batch is NaN, as autograd's would be,
    // not finite garbage (tests/test_stash_formats_gpu.py, tests/test_api_gpu.py::test_on_surface_count_hint).
    bool poison = false;                                // (a divergent bool: one lane-mask SGPR pair, no vector register)
    auto store_fx = [&](int layer) {
        if constexpr (kFx) {
            if constexpr (kColScale) tmax.fs = sb * 0x1p-15f;
            // (the plain columns' forward sweep has no column scale: its array is written once, at the end of the pass)
            // (every lane stores — the four lane quarters of a column the same number to the same address: a store under `if (q == 0)`
            //  splits the last k-block step of every layer into several basic blocks, and the reverse sweeps, which had no such
            //  store before, lost 12-18 % to it: profiles/r05_e_ab.txt)
            if constexpr (kColScale) a.fxs[(int64_t)layer * a.np + p] = poison ? quiet_nan() : inv_sb * 0x1p15f;
        }
    };
    unsigned* lds_amax = reinterpret_cast<unsigned*>(lds + amax_lds_off<H, SW, SP>(a));
    auto publish = [&](int layer) {
        // (layers beyond the table share its last word: only networks of more than kMaxAmaxLayers layers have them, and their
        //  weight-gradient GEMM does not read the table — no uniform branch in the layer-switch step either)
        if constexpr (kRow >= 0) { lds_max_wave(lds_amax + (layer < kMaxAmaxLayers ? layer : kMaxAmaxLayers - 1), tmax.t); tmax.t = 0.f; }
    };
    auto in_layer = [&](int j) -> int { return sweep_in_layer<SW>(a, j); };
    auto bias_ptr = [&](int layer) -> const float* {   // forward sweep: b_{layer+1}
        return a.b1s + (size_t)layer * H;              // [L][H] biases as packed (row 0 = rho b_1)
    };
    auto stash_base = [&](int layer, int T) -> int64_t { return sweep_stash_base(a, layer, T); };
    const unsigned vo = (unsigned)(((int64_t)q * a.np + p) * 16);     // this lane's granule, in bytes
    const LaneOff vl(vo, (is_hess(SW) && !is_jet(SW)) ? (unsigned)(((int64_t)q * a.np + (p >> 2)) * 16) : vo,   // C: one copy per quad
                     P24 ? (unsigned)(((p >> 4) * 64 + lane) * 12) : 0u,                                          // 24-bit tile-major arrays
                     !P24 ? 0u : (is_hess(SW) && !is_jet(SW)) ? (unsigned)(((p >> 6) * 64 + 16 * q + ((p >> 2) & 15)) * 12)   // C there: column p >> 2 of the quad region
                                                              : (unsigned)(((p >> 4) * 64 + lane) * 12));
    auto load_ops = [&](int layer, int kb, TailOps& o) {
        epilogue_loads<SW, FL, P24>(a, stash_base(layer, 2 * kb), vl, o.o1a, o.o2a, o.o3a);
        epilogue_loads<SW, FL, P24>(a, stash_base(layer, 2 * kb + 1), vl, o.o1b, o.o2b, o.o3b);
        if constexpr (BS == SWEEP_FWD && SP != 0) {
            // fp16x3: every layer's bias sits in LDS behind the weight buffers (sweep_body_b) — a vector-memory instruction
            // costs its wave ~100 cycles of issue when the CU's eight waves contend (s_memtime timeline: the two bias loads
            // held the waves that multiply first for 600 cycles of every step), an LDS read 4
            const float* lb = reinterpret_cast<const float*>(lds + 3 * G::CHUNKB) + layer * H + 32 * kb + 4 * q;
            o.ba = *reinterpret_cast<const f32x4*>(lb);
            o.bb = *reinterpret_cast<const f32x4*>(lb + 16);
        } else if constexpr (BS == SWEEP_FWD) {
            o.ba = *reinterpret_cast<const f32x4*>(bias_ptr(layer) + 32 * kb + 4 * q);
            o.bb = *reinterpret_cast<const f32x4*>(bias_ptr(layer) + 32 * kb + 16 + 4 * q);
        }
    };
    // tail of tiles 2kb, 2kb+1 of `layer`: fp32 results (and the stash stores the sweep owes)
    auto run_tail = [&](int layer, int kb, const f32x4 z0, const f32x4 z1, const TailOps& o, f32x4& e0, f32x4& e1) {
        const f32x4 zero = {0, 0, 0, 0};
        if constexpr (BS == SWEEP_FWD && SP != 0 && HS) {   // quads: the bias only in the value channel; `unscale` is this column's
            const f32x4 us = {unscale, unscale, unscale, unscale};
            e0 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, __builtin_elementwise_fma(z0, us, isv ? o.ba : zero), zero, zero, zero, stash_base(layer, 2 * kb), vl, isv, tmax);
            e1 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, __builtin_elementwise_fma(z1, us, isv ? o.bb : zero), zero, zero, zero, stash_base(layer, 2 * kb + 1), vl, isv, tmax);
        } else if constexpr (BS == SWEEP_FWD && SP != 0) {  // plain columns: z = 2^-k (2^k W h) + b, one FMA per value
            // (measured and dropped, round 4: w0 2/pi folded into this FMA and the biases, sin / cos from the argument in quarter
            //  turns — two instructions per value fewer, -2 % on this sweep, value error unchanged; but the ROUNDED constant
            //  w0 2/pi is off by 2e-8, the same way for every pre-activation of the network: a coherent error that the 12-step
            //  beetle trajectory amplified to 1e-3 where the reference's own, unbiased, fp32 roundings stay at 2e-7)
            e0 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, __builtin_elementwise_fma(z0, f32x4{unscale, unscale, unscale, unscale}, o.ba), zero, zero, zero, stash_base(layer, 2 * kb), vl, isv, tmax);
            e1 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, __builtin_elementwise_fma(z1, f32x4{unscale, unscale, unscale, unscale}, o.bb), zero, zero, zero, stash_base(layer, 2 * kb + 1), vl, isv, tmax);
        } else if constexpr (BS == SWEEP_FWD) {      // z = W h + b only in the value channel
            e0 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, z0 + (isv ? o.ba : zero), zero, zero, zero, stash_base(layer, 2 * kb), vl, isv, tmax);
            e1 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, z1 + (isv ? o.bb : zero), zero, zero, zero, stash_base(layer, 2 * kb + 1), vl, isv, tmax);
        } else if constexpr (kColScale) {            // accumulators -> true values first (2^-k_j / sb of the matrix that made them)
            e0 = epilogue<SW, FL, kTrackE, P24, false, TailTrackT<kFx>>(a, z0 * unscale, o.o1a, o.o2a, o.o3a, stash_base(layer, 2 * kb), vl, isv, tmax);
            e1 = epilogue<SW, FL, kTrackE, P24, false, TailTrackT<kFx>>(a, z1 * unscale, o.o1b, o.o2b, o.o3b, stash_base(layer, 2 * kb + 1), vl, isv, tmax);
        } else {
            e0 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, z0, o.o1a, o.o2a, o.o3a, stash_base(layer, 2 * kb), vl, isv, tmax);
            e1 = epilogue<SW, FL, false, P24, false, TailTrackT<kFx>>(a, z1, o.o1b, o.o2b, o.o3b, stash_base(layer, 2 * kb + 1), vl, isv, tmax);
        }
    };
    auto pin_ops = [&](TailOps& o) {                    // make the compiler wait for these loads HERE
        if constexpr (BS == SWEEP_FWD) asm volatile("" : "+v"(o.ba), "+v"(o.bb));
        else asm volatile("" : "+v"(o.o1a), "+v"(o.o2a), "+v"(o.o1b), "+v"(o.o2b));
        if constexpr (SW == SWEEP_ADJ_FWD_H || SW == SWEEP_ADJ_REV_H) asm volatile("" : "+v"(o.o3a), "+v"(o.o3b));
    };

    // chunk stream: chunk c = (matrix c / NKB, k-block c % NKB) lives in LDS buffer c % 3 and is fetched TWO steps
    // ahead.  vmcnt retires in order, so a one-step-ahead DMA would force every stash load and store of the previous
    // step to complete within one step as well; with two steps everything gets two (~3 us, an HBM round trip under load).
    const int total = nhid * G::NKB;
    auto chunk_src = [&](int c) -> const char* {       // c is wave-uniform
        const int j = c / G::NKB;
        return image(j) + (size_t)(c - j * G::NKB) * G::CHUNKB;
    };
    __syncthreads();                                   // every wave is past its last LDS read of the previous tile
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;   // LDS byte offset of the buffers
    const unsigned voff = (unsigned)lane * 16u;
    // Waves 0-3 issue ALL the DMA pieces of a chunk (their own six and their SIMD partner's), waves 4-7 none: a
    // vector-memory instruction stalls its wave's in-order issue for ~100 cycles when the CU's eight waves contend, and the
    // waves that multiply first (4-7, see `late` below) are the ones the step waits for — their chain loses the six pieces,
    // the other half, which idled at the barrier, takes them (-0.9 % on the step; the reverse assignment: no gain).
    // A partial pass with at most four active waves (the last pass of a workgroup's share: at 100 000 points a single wave in
    // 112 workgroups) leaves waves 4-7 idle: they take all the pieces then, the active waves none.
    auto dma2 = [&](const char* src, unsigned dst) {
        if (wave < NWB / 2) {
            const int w = wave & (NWB / 2 - 1);
            dma_issue<H, SP>(src, dst, voff, w); dma_issue<H, SP>(src, dst, voff, w + NWB / 2);
        }
    };
    dma2(chunk_src(0), lds0 + gc * G::CHUNKB);
    dma2(chunk_src(1), lds0 + ((gc + 1) % 3) * G::CHUNKB);
    if (wave >= nact) {                                // same DMA pieces, same barriers, nothing else
        dma_wait_b<0>();
        __syncthreads();
        for (int c = 0; c < total; ++c) {
            const bool more = c + 2 < total;
            if (more) dma2(chunk_src(c + 2), lds0 + ((gc + 2) % 3) * G::CHUNKB);
            gc = (gc + 1) % 3;
            if (more) dma_wait_b<2 * G::NDMA>();       // only this step's pieces may still be in flight (waves 4-7: nothing)
            else dma_wait_b<0>();
            __syncthreads();
        }
        return;
    }

    // ------------------------------ first layer (fp32, K = 3): pre-activations / incoming adjoints of 16 tiles -------
    {
        float b = 0.f, yb = 1.f;
        if constexpr (BS == SWEEP_FWD) b = (q < 3) ? a.x4[p * 4 + q] : 0.f;           // bias is added by the tail
        if constexpr (BS == SWEEP_ADJ_FWD) b = (q < 3) ? a.gbar[p * 4 + q] : 0.f;
        if constexpr (BS == SWEEP_ADJ_REV) yb = a.ybar[p];
        if constexpr (SW == SWEEP_REV_H) yb = isv ? 1.f : 0.f;                         // adot_L^k = 0
        if constexpr (kFx) {                                                           // poisoned column? (store_fx)
            if constexpr (BS == SWEEP_REV) poison = nonfinite(a.y[p]);
            if constexpr (BS == SWEEP_ADJ_REV) poison = nonfinite(a.ybar[p]);
            if constexpr (BS == SWEEP_ADJ_FWD) {
                int bad = nonfinite(b) ? 1 : 0;
                bad |= __shfl_xor(bad, 16); bad |= __shfl_xor(bad, 32);
                poison = bad != 0;
            }
        }
#pragma unroll
        for (int T = 0; T < G::NT; ++T) {
            if constexpr (kFwdDir) prev[T] = mfma16(a.w1b[(16 * T + li) * 4 + q], b, f32x4{0, 0, 0, 0});
            else prev[T] = *reinterpret_cast<const f32x4*>(a.theta + a.off_wo + 16 * T + 4 * q) * yb;
        }
    }

    // ------------------------------ hidden x hidden layers ------------------------------
    // Step c:  [operands of tail c+1 have landed] -> DMA of chunk c+2 -> operand loads of tail c+3 -> 16 tiles x 6
    // MFMAs with B(c), interleaved with tail c+1 -> B(c+1) -> wait for chunk c+1 + barrier.  Tail t = pair t % NKB of
    // the layer feeding matrix t / NKB; the last step of a layer runs the first tail of the next one once its own
    // accumulators are final.
    // Tail operands: plain columns keep two sets (the next tail's, pinned at the top of the step, and the one after it,
    // loaded right behind the DMA: a full step ahead); the quad variants have a third operand array and no registers
    // for that — one set, refilled right after the tail that consumed it (about 0.8 step ahead).
    // (the fp16x3 adjoint forward sweep — two loads, two stores and the column scales — fits its registers with one set only)
    constexpr bool kOneSet = HS;
    TailOps ops_cur, ops_n1;
    u32x4 bp[NPC];                                     // B operand of the current step: bf16 h | m | l, or fp16 hi | lo
    auto split = [&](const f32x4 e0, const f32x4 e1, u32x4 (&o)[NPC]) {
        if constexpr (kColScale) split8h(e0 * sb, e1 * sb, o[0], o[1]);
        else if constexpr (SP) split8h(e0, e1, o[0], o[1]);
        else split8(e0, e1, o[0], o[1], o[2]);
    };
    // per layer and column max_f |e_l|: the adjoint forward sweep leaves it for the adjoint reverse sweep's column scale
    auto store_ebound = [&](int layer) {
        if constexpr (kTrackE) {                         // (every lane stores, no branch: see store_fx; the training launches always pass ebound)
            float m = fmaxf(tmax.e, __shfl_xor(tmax.e, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            a.ebound[(int64_t)layer * a.np + p] = m;
            tmax.e = 0.f;
        }
    };
    f32x4 fin0 = {0, 0, 0, 0}, fin1 = {0, 0, 0, 0};    // fp32 results of pair 0 of the layer after the last matrix
    load_ops(in_layer(0), 0, ops_cur);
    if constexpr (!kOneSet) load_ops(in_layer(0), 1, ops_n1);
    if constexpr (kColScale) {                         // first layer (fp32 MFMA / W_out^T ybar: true values): its column scale
        const float eb0 = ebound_of(in_layer(0)), zb0 = zbound_of(in_layer(0));
        if (nhid > 0) { eb_next = ebound_of(in_layer(1)); zb_next = zbound_of(in_layer(1)); }
        const float cm = col_absmax(prev);
        store_zbound(in_layer(0), cm);
        set_scale(cm, eb0, zb0);
    }
    store_fx(in_layer(0));
    {
        f32x4 e0, e1;
        run_tail(in_layer(0), 0, prev[0], prev[1], ops_cur, e0, e1);
        split(e0, e1, bp);
        if constexpr (kOneSet) load_ops(in_layer(0), 1, ops_cur);
    }
#pragma unroll
    for (int T = 0; T < G::NT; ++T) acc[T] = f32x4{0, 0, 0, 0};
    dma_wait_b<0>();                                   // once per tile: chunks 0 and 1 and everything above
    __syncthreads();
    constexpr int kYoung = younger_ops<SW, FL>() - ((SP != 0 && BS == SWEEP_FWD) ? 2 : 0);   // fp16x3 forward: the bias comes from LDS
    // The two waves of a SIMD (w, w + 4) leave every k-block barrier together.  With the same program order both run
    // their tail (vector ALU) at the same time and then collide on the matrix pipe: the step costs tail + MFMAs of both.
    // Waves 4-7 therefore run their MFMAs FIRST and the tail of the next step behind them (the tail only needs the
    // previous layer's accumulators, not this step's): each half's tail falls beside the other half's MFMAs.
    // (also for the Hessian-quad variants that keep their registers: the adjoint-forward quads and the jets would spill)
    constexpr bool kLateOk = !HS || (SW != SWEEP_ADJ_FWD_H && SW != SWEEP_FWD_J);
    #ifdef DUDF_LATE_FORCE                                 // tests/isa_contract.py: one half's program order at a time, branch-free
    const bool late = kLateOk && DUDF_LATE_FORCE;
#else
    const bool late = kLateOk && __builtin_amdgcn_readfirstlane((int)(wave >= NWB / 2)) != 0;
#endif
    // feed slot: after which tile's MFMAs a wave issues its DMA pieces and operand loads (-1: at the top of the step);
    // tail slot: after which tile's MFMAs it runs the tail of the next step.  A = waves 0-3, B = waves 4-7 (when `late`).
    constexpr int FA = -1, TA = 0, FB = (BS == SWEEP_FWD ? 15 : 7) * (G::NT - 1) / 15, TB = G::NT - 1;
    for (int j = 0; j < nhid; ++j) {
        const int lin = in_layer(j), lnx = in_layer(j + 1);
#pragma unroll
        for (int kb = 0; kb < G::NKB; ++kb) {
            const int c = j * G::NKB + kb;
            const char* bpl = lds + gc * G::CHUNKB + lane * 16;
            auto frag = [&](int T, int pc) -> u32x4 {
                return *reinterpret_cast<const u32x4*>(bpl + (T * NPC + pc) * G::FRAG);
            };
            if constexpr (!kOneSet) ops_cur = ops_n1;
            pin_ops(ops_cur);
            const bool more = c + 2 < total;
            auto load_after_next = [&](TailOps& o) {                 // operands of tail c+2
                if (kb + 2 < G::NKB) load_ops(lin, kb + 2, o);
                else load_ops(lnx, kb + 2 - G::NKB, o);
            };
            auto feed = [&]() {                                      // this step's DMA pieces, then the operand loads
                if (more) dma2(chunk_src(c + 2), lds0 + ((gc + 2) % 3) * G::CHUNKB);
                if constexpr (!kOneSet) load_after_next(ops_n1);          // one full step ahead
            };
            u32x4 nb[NPC];
            // fp16x3: the half that does not multiply first runs its tail at the very top of the step, in front of its DMA
            // pieces (fetched two steps ahead: no hurry) and of its first LDS fragment: the step is (tail of one half beside the
            // MFMAs of the other) twice, and neither tail should wait for anything
            constexpr bool kTailTop = SP != 0 && BS == SWEEP_FWD;
            if (kTailTop && !late && kb + 1 < G::NKB) {
                f32x4 e0, e1;
                run_tail(lin, kb + 1, prev[2 * kb + 2], prev[2 * kb + 3], ops_cur, e0, e1);
                split(e0, e1, nb);
                if constexpr (kOneSet) load_after_next(ops_cur);
                __builtin_amdgcn_sched_barrier(0);
            }
            if ((FA < 0 && !late) || (FB < 0 && late)) feed();
            __builtin_amdgcn_sched_barrier(0);
            // A fragments travel two tiles (12 MFMAs, ~190 cycles) ahead of their use: with both waves of a SIMD and the
            // chunk DMA on the LDS, one tile of distance does not cover the read latency
            // (fp16x3: FOUR tiles = 12 MFMAs: a tile is only three MFMAs long)
            constexpr int AD = (SP && BS == SWEEP_FWD) ? 4 : 2;   // (the other fp16x3 sweeps need the registers: two tiles)
            u32x4 an[AD][NPC];
#pragma unroll
            for (int T = 0; T < AD; ++T)
#pragma unroll
                for (int pc = 0; pc < NPC; ++pc) an[T][pc] = frag(T, pc);
            // TP tiles per trip, their MFMA chains interleaved: a tile's products accumulate into ONE register quad, and a
            // wave that issues them back to back waits out each MFMA's latency (fp16x3: three-instruction chains — alone on
            // the pipe a wave reached one MFMA per ~34 cycles instead of 16)
            constexpr int TP = SP ? 2 : 1;
#pragma unroll
            for (int T = 0; T < G::NT; T += TP) {
                u32x4 af[TP][NPC];
#pragma unroll
                for (int u = 0; u < TP; ++u)
#pragma unroll
                    for (int pc = 0; pc < NPC; ++pc) af[u][pc] = an[(T + u) % AD][pc];
                if (T + AD < G::NT) {
#pragma unroll
                    for (int u = 0; u < TP; ++u)
#pragma unroll
                        for (int pc = 0; pc < NPC; ++pc) an[(T + u) % AD][pc] = frag(T + u + AD, pc);
                    // vector/scalar ALU and vector memory may move across, LDS reads and MFMAs may not: otherwise hipcc
                    // floats each tile's MFMAs up to its reads and every fragment is waited for just in time
                    __builtin_amdgcn_sched_barrier(0x76);
                }
                f32x4 cc[TP];
#pragma unroll
                for (int u = 0; u < TP; ++u) cc[u] = acc[T + u];
                mma_products<SP, TP, NPC>(af, bp, cc);
#pragma unroll
                for (int u = 0; u < TP; ++u) acc[T + u] = cc[u];
                const int Tl = T + TP - 1;                              // last tile of this trip
                if ((FA >= T && FA <= Tl && !late) || (FB >= T && FB <= Tl && late)) {   // the late half issues its DMA pieces (60-180 cycles
                    __builtin_amdgcn_sched_barrier(0);                  // of issue each) under the other half's MFMAs
                    feed();
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (kb + 1 < G::NKB && ((TA >= T && TA <= Tl && !late && !kTailTop) || (TB >= T && TB <= Tl && late))) {   // the next step's B operand
                    if (T != 0) __builtin_amdgcn_sched_barrier(0);
                    f32x4 e0, e1;
                    run_tail(lin, kb + 1, prev[2 * kb + 2], prev[2 * kb + 3], ops_cur, e0, e1);
                    split(e0, e1, nb);
                    if constexpr (kOneSet) load_after_next(ops_cur);
                }
            }
            if (kb + 1 == G::NKB) {                                     // layer done: first tail of the next one
                if constexpr (kColScale) {
                    // this matrix consumed the operand scaled by sb: its accumulators are 2^k_j sb x the true values
                    unscale = unscale_of(j) * inv_sb;
                    const float ebl = eb_next, zbl = zb_next;
                    // a layer ahead: its latency hides behind 8 steps.  (No branch at the end of the stream: the last switches re-read the
                    // last layer's entry — a uniform branch would end the basic block of this step as well, see store_fx)
                    { const int jn = j + 2 <= nhid ? j + 2 : nhid; eb_next = ebound_of(in_layer(jn)); zb_next = zbound_of(in_layer(jn)); }
                    const float cm = col_absmax(acc) * unscale;
                    store_zbound(lnx, cm);
                    set_scale(cm, ebl, zbl);                            // ... and the scale of the operand its tails are about to build
                } else if constexpr (SP) unscale = unscale_of(j);
                store_fx(lnx);
                publish(lin);                                           // every tail of layer `lin` has run
                store_ebound(lin);
                run_tail(lnx, 0, acc[0], acc[1], ops_cur, fin0, fin1);
                split(fin0, fin1, nb);
                if constexpr (kOneSet) load_after_next(ops_cur);
#pragma unroll
                for (int T = 0; T < G::NT; ++T) { prev[T] = acc[T]; acc[T] = f32x4{0, 0, 0, 0}; }
            }
#pragma unroll
            for (int pc = 0; pc < NPC; ++pc) bp[pc] = nb[pc];
            gc = (gc + 1) % 3;
            // chunk c+1 landed; c+2 and two steps' stash traffic stay in flight.  Only the waves that issued DMA pieces wait
            // (0-3: the barrier behind publishes the chunk to the others)
            // (tail at the top of the step: its stores are OLDER than this step's pieces — one step of stash traffic less)
            if (more) { if (wave < NWB / 2) dma_wait_b<(kTailTop ? 1 : 2) * kYoung + 2 * G::NDMA>(); }
            else dma_wait_b<0>();
            __syncthreads();
        }
    }

    // ------------------------------ remaining tails of the last hidden layer + output stage (fp32) -------------------
    {
        const int lin = in_layer(nhid);
        float part = 0.f;
        f32x4 accg = {0, 0, 0, 0};
#pragma unroll
        for (int kb = 0; kb < G::NKB; ++kb) {
            f32x4 e0 = fin0, e1 = fin1;
            if (kb > 0) {
                if constexpr (!kOneSet) {
                    ops_cur = ops_n1;
                    if (kb + 1 < G::NKB) load_ops(lin, kb + 1, ops_n1);
                }
                run_tail(lin, kb, prev[2 * kb], prev[2 * kb + 1], ops_cur, e0, e1);
                if constexpr (kOneSet) { if (kb + 1 < G::NKB) load_ops(lin, kb + 1, ops_cur); }
            }
            if constexpr (BS == SWEEP_REV) {
                // (own copy of out_tile / out_grad, dudf_sweep16.h: through them the default step's reverse sweep took 0.5060 ms (median of
                //  three) against the parent's 0.5036 + 0.0006 of spread, MI355X, profiles/HISTORY.md)
                const f32x4 w0v = *reinterpret_cast<const f32x4*>(a.w1t16 + li * H + 32 * kb + 4 * q);
                const f32x4 w1v = *reinterpret_cast<const f32x4*>(a.w1t16 + li * H + 32 * kb + 16 + 4 * q);
#pragma unroll
                for (int t = 0; t < 4; ++t) accg = mfma16(w0v[t], e0[t], accg);
#pragma unroll
                for (int t = 0; t < 4; ++t) accg = mfma16(w1v[t], e1[t], accg);
            } else {
                out_tile<BS, H>(a, 2 * kb, li, q, e0, part, accg);
                out_tile<BS, H>(a, 2 * kb + 1, li, q, e1, part, accg);
            }
        }
        publish(lin);
        store_ebound(lin);
        if constexpr (BS == SWEEP_REV) {
            if constexpr (kFx) { if (poison) accg = f32x4{quiet_nan(), quiet_nan(), quiet_nan(), 0.f}; }   // df/dx of a poisoned column (its cos came back as a finite number)
            if (q == 0) *reinterpret_cast<f32x4*>(a.g + p * 4) = f32x4{accg[0], accg[1], accg[2], 0.f};
        } else out_finish<BS, kFx, kColScale>(a, p, q, isv, part, accg, poison);
    }
}

// ---- "oct mode": a pass that holds ONE 16-column group (the last pass of a workgroup's share: at 100 000 points 112 of the 256
// workgroups end with one) ---------------------------------------------------------------------------------------------------
// With sweep_tile_b a lone wave does everything serially: 8 tails and 8 x 48 MFMAs per layer, nothing to overlap them with
// (measured in situ: 0.19 ms of a 3.2 ms step; alone, a lone-wave pass takes 0.68 of a full one).  Here all eight waves share
// the group: wave w owns output tiles 2w, 2w+1 — exactly the pair whose post-tail values are the B operand of k-block w of
// the next matrix.  Per layer: [column scale: max over the waves' 32 features each, through LDS] -> every wave runs ONE
// tail pair (in parallel: an eighth of the lone wave's tail work) and publishes its B fragment (hi | lo, 2 KiB) in LDS ->
// 8 k-blocks of 6 MFMAs per wave, B(kb) read from LDS.  fp16x3, plain columns, H = 256.  No weight chunks through LDS here: a
// wave needs only ITS two tiles' fragments (4 KiB of a 32 KiB chunk), so it loads them from L2 straight into registers — all
// 32 fragments of a layer at the top of the layer, behind the exchange and the tail (a step of 6 MFMAs is far shorter than
// an LDS-DMA round trip: with the chunk stream the pass was bound by DMA latency).  Two barriers per layer, no hand-counted
// waits; the chunk buffers and `gc` are left alone.
template <int H, int SW, int FL, int P24 = 0>
__device__ __forceinline__ void sweep_tile_oct(const SweepArgs& a, const int g, char* lds, unsigned& gc, const unsigned oct_off) {
    using G = GeoB<H, 1>;
    static_assert(H == 256 && SW <= SWEEP_ADJ_REV, "fp16x3, plain columns, one k-block per wave");
    constexpr int NPC = 2;
    constexpr int BS = base_of(SW);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, q = lane >> 4;
    const int nhid = a.L - 1;
    constexpr bool kFwdDir = fwd_dir<SW>();
    constexpr bool kColScale = BS != SWEEP_FWD;
    constexpr bool kTrackE = BS == SWEEP_ADJ_FWD;
    constexpr int kRow = amax_row<SW, FL>();
    const int64_t p = (int64_t)g * 16 + li;
    const int T0 = 2 * wave;
    auto image = [&](int j) -> const char* { return sweep_image<SW, G::IMGB, 1>(a, nhid, j); };
    auto unscale_of = [&](int j) -> float { return sweep_unscale<SW>(a, nhid, j); };
    auto in_layer = [&](int j) -> int { return sweep_in_layer<SW>(a, j); };
    auto stash_base = [&](int layer, int T) -> int64_t { return sweep_stash_base(a, layer, T); };
    const LaneOff vo((unsigned)(((int64_t)q * a.np + p) * 16), (unsigned)(((int64_t)q * a.np + p) * 16),
                     P24 ? (unsigned)(((p >> 4) * 64 + lane) * 12) : 0u);
    char* ox = lds + oct_off;
    u32x4* Bx = reinterpret_cast<u32x4*>(ox);                          // [k-block][piece][lane]
    float* cmx = reinterpret_cast<float*>(ox + 8 * NPC * 1024);        // [wave][column]: max |accumulator|
    float* emx = cmx + 128;                                            // [wave][column]: max |e_l| (adjoint forward sweep)
    f32x4* red = reinterpret_cast<f32x4*>(ox + 8 * NPC * 1024 + 1024); // [wave][lane]: output-stage partial sums
    unsigned* lds_amax = reinterpret_cast<unsigned*>(lds + 3 * G::CHUNKB);

    (void)gc;
    __syncthreads();                                   // every wave is past its last LDS read of the previous pass

    // first layer (fp32, K = 3): my two tiles
    f32x4 prev[2], acc[2];
    bool poison = false;
    {
        float b = 0.f, yb = 1.f;
        if constexpr (BS == SWEEP_FWD) b = (q < 3) ? a.x4[p * 4 + q] : 0.f;
        if constexpr (BS == SWEEP_ADJ_FWD) b = (q < 3) ? a.gbar[p * 4 + q] : 0.f;
        if constexpr (BS == SWEEP_ADJ_REV) yb = a.ybar[p];
        if constexpr ((P24 & 1) != 0) {                 // poisoned column? (sweep_tile_b: store_fx)
            if constexpr (BS == SWEEP_REV) poison = nonfinite(a.y[p]);
            if constexpr (BS == SWEEP_ADJ_REV) poison = nonfinite(yb);
            if constexpr (BS == SWEEP_ADJ_FWD) {
                int bad = nonfinite(b) ? 1 : 0;
                bad |= __shfl_xor(bad, 16); bad |= __shfl_xor(bad, 32);
                poison = bad != 0;
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int T = T0 + u;
            if constexpr (kFwdDir) prev[u] = mfma16(a.w1b[(16 * T + li) * 4 + q], b, f32x4{0, 0, 0, 0});
            else prev[u] = *reinterpret_cast<const f32x4*>(a.theta + a.off_wo + 16 * T + 4 * q) * yb;
        }
    }
    f32x4 o1[2], o2[2], o3[2], bs[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    auto load_ops = [&](int layer) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            epilogue_loads<SW, FL, P24>(a, stash_base(layer, T0 + u), vo, o1[u], o2[u], o3[u]);
            if constexpr (BS == SWEEP_FWD)
                bs[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(lds + 3 * G::CHUNKB) + layer * H + 16 * (T0 + u) + 4 * q);
        }
    };
    auto ebound_of = [&](int layer) -> float {
        if constexpr (BS == SWEEP_ADJ_REV && (FL & 1) != 0) return a.ebound[(int64_t)layer * a.np + p];
        return 0.f;
    };
    load_ops(in_layer(0));
    float eb = ebound_of(in_layer(0));
    float unscale = 1.f, sb = 1.f, inv_sb = 1.f;
    constexpr bool kFx = (P24 & 1) != 0;
    TailTrackT<kFx> tk;
    f32x4 e[2];
    for (int j = 0; j <= nhid; ++j) {
        const int lin = in_layer(j);
        if constexpr (kColScale) {                      // the column's scale from ALL 16 tiles: max over the eight waves
            const float m = col_absmax(prev);
            if (q == 0) cmx[wave * 16 + li] = m;
            __syncthreads();
            float mm = 0.f;
#pragma unroll
            for (int w = 0; w < NWB; ++w) mm = fmaxf(mm, cmx[w * 16 + li]);
            col_scale(plain_bound(a.w0, mm * unscale, eb) * DUDF_FX_HEADROOM, sb, inv_sb);   // (2^-10 of head room: see set_scale)
        }
        if constexpr (kFx) {                            // fixed-point stash: this layer's column scale for the readers
            if constexpr (kColScale) tk.fs = sb * 0x1p-15f;
            if (wave == 0 && q == 0) a.fxs[(int64_t)lin * a.np + p] = poison ? quiet_nan() : (kColScale ? inv_sb * 0x1p15f : 1.f);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {                   // ONE tail pair per wave and layer
            f32x4 z = prev[u];
            if constexpr (BS == SWEEP_FWD) z = __builtin_elementwise_fma(z, f32x4{unscale, unscale, unscale, unscale}, bs[u]);
            else z *= unscale;
            e[u] = epilogue<SW, FL, kTrackE, P24, false, TailTrackT<kFx>>(a, z, o1[u], o2[u], o3[u], stash_base(lin, T0 + u), vo, true, tk);
        }
        if constexpr (kRow >= 0) { if (lin < kMaxAmaxLayers) lds_max_wave(lds_amax + lin, tk.t); tk.t = 0.f; }
        if constexpr (kTrackE) {
            float m = fmaxf(tk.e, __shfl_xor(tk.e, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            if (q == 0) emx[wave * 16 + li] = m;
            tk.e = 0.f;
        }
        if (j == nhid) break;
        // this wave's A fragments of matrix j: [k-block][tile][piece], 16 B per lane each
        u32x4 fr[G::NKB][2][NPC];
        {
            const char* img = image(j) + (size_t)lane * 16;
#pragma unroll
            for (int kb = 0; kb < G::NKB; ++kb)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int pc = 0; pc < NPC; ++pc)
                        fr[kb][u][pc] = *reinterpret_cast<const u32x4*>(img + (size_t)kb * G::CHUNKB + ((T0 + u) * NPC + pc) * G::FRAG);
        }
        u32x4 bh, bl;
        if constexpr (kColScale) split8h(e[0] * sb, e[1] * sb, bh, bl);
        else split8h(e[0], e[1], bh, bl);
        Bx[(wave * NPC + 0) * 64 + lane] = bh;          // = the B operand of k-block `wave` of matrix j
        Bx[(wave * NPC + 1) * 64 + lane] = bl;
        load_ops(in_layer(j + 1));                      // the next layer's tail operands: a whole k-loop ahead
        eb = ebound_of(in_layer(j + 1));
        __syncthreads();
        if constexpr (kTrackE) {                        // per layer and column max_f |e_l| for the adjoint reverse sweep
            if (wave == 0 && q == 0 && a.ebound) {
                float m = 0.f;
#pragma unroll
                for (int w = 0; w < NWB; ++w) m = fmaxf(m, emx[w * 16 + li]);
                a.ebound[(int64_t)lin * a.np + p] = m;
            }
        }
        acc[0] = f32x4{0, 0, 0, 0}; acc[1] = acc[0];
#pragma unroll
        for (int kb = 0; kb < G::NKB; ++kb) {
            const u32x4 bx[NPC] = {Bx[(kb * NPC + 0) * 64 + lane], Bx[(kb * NPC + 1) * 64 + lane]};
#pragma unroll
            for (int u = 0; u < 2; ++u) mma_products<1, 1, NPC>(&fr[kb][u], bx, &acc[u]);
        }
        __syncthreads();                                // every wave has read B: the next layer may overwrite it
        prev[0] = acc[0]; prev[1] = acc[1];
        unscale = kColScale ? unscale_of(j) * inv_sb : unscale_of(j);
    }
    // output stage: the eight waves' partial results through LDS
    float part = 0.f;
    f32x4 accg = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 2; ++u) out_tile<BS, H>(a, T0 + u, li, q, e[u], part, accg);
    if constexpr (BS == SWEEP_FWD) {
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (q == 0) cmx[wave * 16 + li] = part;
        __syncthreads();
        if (wave == 0 && q == 0) {
            float y = a.theta[a.off_bo];
#pragma unroll
            for (int w = 0; w < NWB; ++w) y += cmx[w * 16 + li];
            a.y[p] = y;
            if constexpr (kFx) { if (nonfinite(y)) out_fxs(a, p, quiet_nan()); }
        }
    } else if constexpr (BS == SWEEP_REV) {
        red[wave * 64 + lane] = accg;
        __syncthreads();
        if (wave == 0 && q == 0) {
            f32x4 sum = {0, 0, 0, 0};
#pragma unroll
            for (int w = 0; w < NWB; ++w) sum += red[w * 64 + lane];
            out_grad<kFx>(a, p, sum, poison);
        }
    } else if constexpr (kTrackE) {                     // the last layer's max |e_l|
        __syncthreads();
        if (wave == 0 && q == 0 && a.ebound) {
            float m = 0.f;
#pragma unroll
            for (int w = 0; w < NWB; ++w) m = fmaxf(m, emx[w * 16 + li]);
            a.ebound[(int64_t)in_layer(nhid) * a.np + p] = m;
        }
    }
}

// (bid, nblk): this workgroup's index among the `nblk` that share the columns of `a` — the whole grid, or one of the two
// parts of a pair launch (sweep_pair_kernel)
// (sweep_w_body, dudf_sweep_wide.hip, is the same driver — clock, amax init and flush, shares.  As one function that takes the pass as
//  a lambda it changed 35 of 35 and 74 of 94 kernels, with more scratch in 11 of them — outside the per-kernel limit: tools/asm_diff.py.)
template <int H, int SW, int FL, int SP = 0, int P24 = 0>
__device__ __forceinline__ void sweep_body_b(const SweepArgs& a, const int bid, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char lds_b[];
    unsigned gc = 0;
    const bool clk_on = a.clk != nullptr && bid == 0;   // profiling: the clock this kernel runs at
    const unsigned long long clk_t0 = clk_on ? __builtin_amdgcn_s_memtime() : 0ull, clk_r0 = clk_on ? __builtin_amdgcn_s_memrealtime() : 0ull;
    constexpr int kRow = amax_row<SW, FL>();
    unsigned* lds_amax = reinterpret_cast<unsigned*>(lds_b + amax_lds_off<H, SW, SP>(a));
    if constexpr (kRow >= 0) { if (threadIdx.x < kMaxAmaxLayers) lds_amax[threadIdx.x] = 0u; }   // (sweep_tile_b starts with a barrier)
    if constexpr (SP != 0 && base_of(SW) == SWEEP_FWD) {     // b_1 .. b_L behind the three weight buffers (read by the tails)
        float* lb = reinterpret_cast<float*>(lds_b + 3 * GeoB<H, SP>::CHUNKB);
        for (int i = threadIdx.x; i < a.L * H; i += 64 * NWB) lb[i] = a.b1s[i];      // [L][H] biases as packed (row 0 = rho b_1)
    }
    // balanced shares of 16-column groups; a share is walked in passes of 8 groups, the last one possibly partial —
    // a pass with one wave per SIMD (or a single wave) costs about half a full one, a whole extra round would cost all of it
    const int ng = a.ntiles * (TILE / 16), gbase = a.tile0 * (TILE / 16);
    const int g0 = (int)((int64_t)bid * ng / nblk), g1 = (int)((int64_t)(bid + 1) * ng / nblk);
    constexpr bool kOct = SP != 0 && H == 256 && SW <= SWEEP_ADJ_REV;
    for (int g = g0; g < g1; g += NWB) {
        if constexpr (kOct) {
            if (g1 - g == 1) {                          // a pass with one group: all eight waves share it
                const unsigned oct_off = 3 * GeoB<H, SP>::CHUNKB + (base_of(SW) == SWEEP_FWD ? (unsigned)(a.L * H * sizeof(float)) : (unsigned)(kMaxAmaxLayers * sizeof(unsigned)));
                sweep_tile_oct<H, SW, FL, P24>(a, gbase + g, lds_b, gc, oct_off);
                continue;
            }
        }
        sweep_tile_b<H, SW, FL, SP, P24>(a, gbase + g, (g1 - g < NWB) ? g1 - g : NWB, lds_b, gc);
    }
    if constexpr (kRow >= 0) {
        __syncthreads();
        if ((int)threadIdx.x < a.L && (int)threadIdx.x < kMaxAmaxLayers && a.amax) {
            const unsigned v = lds_amax[threadIdx.x];
            if (v) atomicMax(a.amax + kRow * a.L + threadIdx.x, v);
        }
    }
    if (clk_on && threadIdx.x == 0) {
        a.clk[0] = __builtin_amdgcn_s_memtime() - clk_t0;
        a.clk[1] = __builtin_amdgcn_s_memrealtime() - clk_r0;
    }
}
// Two code generations of the same body.  The packed fp32 instructions (v_pk_fma_f32 ...) halve the vector-ALU issue
// slots of a tail, but they do not execute beside the SIMD partner's MFMAs (tools/micro/coissue.hip: 48 v_pk_fma_f32 +
// 24 MFMAs take the SUM of their times, 48 v_fma_f32 + 24 MFMAs the maximum + 25 %).  The forward sweep, whose sin/cos
// tail is as long as its MFMA stream, is therefore built WITHOUT them and overlaps the two; the other sweeps (short
// tails, bound by the stash stream) keep them.
// (the Hessian-quad and jet variants too: +3 % / +5 % on the Hessian-frame and curvature queries)
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_bf16_kernel(SweepArgs a) { sweep_body_b<H, SW, FL>(a, blockIdx.x, gridDim.x); }
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) DUDF_NO_PK void sweep_bf16_np_kernel(SweepArgs a) { sweep_body_b<H, SW, FL>(a, blockIdx.x, gridDim.x); }
// the fp16x3 builds (own names: tests/isa_contract.py tells the two families apart by them)
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_f16_kernel(SweepArgs a) { sweep_body_b<H, SW, FL, 1>(a, blockIdx.x, gridDim.x); }
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) DUDF_NO_PK void sweep_f16_np_kernel(SweepArgs a) { sweep_body_b<H, SW, FL, 1>(a, blockIdx.x, gridDim.x); }
// ... and the fp16x3 builds that keep stash arrays at 24 bits, tile-major (dudf_internal.h "p24"; training variants):
// f16r: R, E and C (stash mask 6); f16p: S, Q, A, Z as well (mask 7, the default stash of 256-wide networks)
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_f16r_kernel(SweepArgs a) { sweep_body_b<H, SW, FL, 1, 6>(a, blockIdx.x, gridDim.x); }
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) DUDF_NO_PK void sweep_f16r_np_kernel(SweepArgs a) { sweep_body_b<H, SW, FL, 1, 6>(a, blockIdx.x, gridDim.x); }
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_f16p_kernel(SweepArgs a) { sweep_body_b<H, SW, FL, 1, 7>(a, blockIdx.x, gridDim.x); }
template <int H, int SW, int FL>
__global__ __launch_bounds__(64 * NWB) DUDF_NO_PK void sweep_f16p_np_kernel(SweepArgs a) { sweep_body_b<H, SW, FL, 1, 7>(a, blockIdx.x, gridDim.x); }
// Pair launch (a batch with Hessian-path points: `loss_s1` with its eigenvector term, the reference's shipped recipe).  A sweep
// then has two column ranges — the quads (variant SWQ; fp16x3 or, SPQ = 0, bf16x6) and the plain columns (fp16x3, variant SWP) — which used to be
// two launches of <= 256 persistent workgroups each: at the reference's batch (29 970 points = 312 + 156 tiles of 128 columns)
// that is 1.2 rounds + 0.6 rounds, each rounded up by the tail of its own launch.  Here ONE grid carries both: the first
// `nbq` workgroups walk the quads, the rest the plain columns, and the host splits the 256 workgroups so that both parts
// finish together (launch_pair).  The two bodies are the ones above, unchanged.
template <int H, int SWQ, int FLQ, int SWP, int FLP, int SPQ, int P24 = 0>
__global__ __launch_bounds__(64 * NWB) DUDF_NO_PK void sweep_pair_kernel(SweepArgs aq, SweepArgs ap, int nbq) {
    if ((int)blockIdx.x < nbq) sweep_body_b<H, SWQ, FLQ, SPQ, P24>(aq, blockIdx.x, nbq);
    else sweep_body_b<H, SWP, FLP, 1, P24>(ap, (int)blockIdx.x - nbq, (int)gridDim.x - nbq);
}

// the instantiation of a family: the forward, Hessian-quad and jet sweeps are the builds without packed fp32 instructions
template <int H, int FAM, int SW, int FL>
constexpr auto sweep_kernel_of() {
    constexpr bool np = sweep_no_pk<SW>();
    if constexpr (FAM == DUDF_FAM_BF16) { if constexpr (np) return &sweep_bf16_np_kernel<H, SW, FL>; else return &sweep_bf16_kernel<H, SW, FL>; }
    else if constexpr (FAM == DUDF_FAM_F16) { if constexpr (np) return &sweep_f16_np_kernel<H, SW, FL>; else return &sweep_f16_kernel<H, SW, FL>; }
    else if constexpr (FAM == DUDF_FAM_F16R) { if constexpr (np) return &sweep_f16r_np_kernel<H, SW, FL>; else return &sweep_f16r_kernel<H, SW, FL>; }
    else { if constexpr (np) return &sweep_f16p_np_kernel<H, SW, FL>; else return &sweep_f16p_kernel<H, SW, FL>; }
}
static_assert(dudf_chunk_bytes(256, 3) == GeoB<256>::CHUNKB && dudf_chunk_bytes(128, 2) == GeoB<128, 1>::CHUNKB, "dudf_variants.h: LDS sizes");
template <int H>
int launch_b(const SweepChoice& c, const SweepArgs& a, hipStream_t st) {
    if (a.ntiles <= 0) return 0;
    const int ntb = (a.ntiles * TILE + TILEB - 1) / TILEB;
    const dim3 grid(ntb < 256 ? ntb : 256), block(GeoB<H>::NTHR);     // one resident 8-wave workgroup per CU
    return dudf_with_variant(kSweepVariants, c.sw, c.fl, [&](auto i) {
        constexpr DudfVariant v = kSweepVariants[decltype(i)::value];
        if (c.family == DUDF_FAM_BF16) return dudf_launch_kernel<sweep_kernel_of<H, DUDF_FAM_BF16, v.sw, v.fl>()>(grid, block, c.lds, c.lds_max, st, a);
        if (c.family == DUDF_FAM_F16) return dudf_launch_kernel<sweep_kernel_of<H, DUDF_FAM_F16, v.sw, v.fl>()>(grid, block, c.lds, c.lds_max, st, a);
        if constexpr (H == 256 && v.p24 != 0) {          // 24-bit tile-major stash: the training variants have a build of their own
            if (c.family == DUDF_FAM_F16R) return dudf_launch_kernel<sweep_kernel_of<H, DUDF_FAM_F16R, v.sw, v.fl>()>(grid, block, c.lds, c.lds_max, st, a);
            if (c.family == DUDF_FAM_F16P) return dudf_launch_kernel<sweep_kernel_of<H, DUDF_FAM_F16P, v.sw, v.fl>()>(grid, block, c.lds, c.lds_max, st, a);
        }
        return (int)DUDF_E_UNSUPPORTED;
    });
}

// Estimated duration of one part of a pair launch, in full plain-column passes: every workgroup walks ceil(ng / nb) groups of 16
// columns in passes of 8 (one per wave); a partial pass with up to one wave per SIMD costs about half a full one (measured: a
// lone wave 0.68, the passes are bound by latency, not by issue), more waves in proportion.  `c` = a pass of this variant
// against a pass of the plain fp16x3 sweep (quads on bf16x6: 1.3-1.65 measured at 29 970 points; 1.5 here).
double pair_est(int ng, int nb, double c) {
    const int m = (ng + nb - 1) / nb, full = m / NWB, rem = m % NWB;
    const double part = rem == 0 ? 0.0 : (rem <= NWB / 2 ? 0.55 : 0.55 + 0.45 * (rem - NWB / 2) / (NWB / 2));
    return c * (full + part);
}
}  // namespace

// One launch for the quad columns (variant base + 4) AND the plain columns (variant base, fp16x3) of a training sweep at H = 256
// (dudf_choose_pair; option pair_launch = 0 switches it off).  The host splits the 256 workgroups so that both parts finish together.
int dudf_launch_sweep_pair(const SweepChoice& c, const SweepArgs& aq, const SweepArgs& ap, hipStream_t st) {
    const int ngq = aq.ntiles * (TILE / 16), ngp = ap.ntiles * (TILE / 16);
    const int tq = (ngq + NWB - 1) / NWB, tp = (ngp + NWB - 1) / NWB;          // passes of 8 groups
    int nbq, nbp;
    if (tq + tp <= 256) { nbq = tq; nbp = tp; }
    else {
        double best = 1e30; nbq = 128;
        for (int q = 1; q < 256; ++q) {
            const double eq = pair_est(ngq, q, 1.5), ep = pair_est(ngp, 256 - q, 1.0);
            const double t = (eq > ep ? eq : ep) + 1e-3 * (eq > ep ? eq - ep : ep - eq);
            if (t < best) { best = t; nbq = q; }
        }
        nbp = 256 - nbq;
    }
    const dim3 grid(nbq + nbp), block(GeoB<256>::NTHR);
    return dudf_with_variant(kPairVariants, c.sw, c.fl, [&](auto i) {
        constexpr DudfVariant v = kPairVariants[decltype(i)::value];
        auto go = [&](auto spq, auto p24) {
            return dudf_launch_kernel<&sweep_pair_kernel<256, v.sw + 4, dudf_pair_flq(v.sw), v.sw, v.fl, decltype(spq)::value, decltype(p24)::value>>(
                grid, block, c.lds, c.lds_max, st, aq, ap, nbq);
        };
        using std::integral_constant;
        if (c.p24 == 7) return go(integral_constant<int, 1>{}, integral_constant<int, 7>{});
        if (c.p24 == 6) return go(integral_constant<int, 1>{}, integral_constant<int, 6>{});
        if (c.spq) return go(integral_constant<int, 1>{}, integral_constant<int, 0>{});
        return go(integral_constant<int, 0>{}, integral_constant<int, 0>{});
    });
}

int dudf_launch_sweep_bf16(const SweepChoice& c, const SweepArgs& a, hipStream_t st) {
    switch (c.H) {
        case 256: return launch_b<256>(c, a, st);
        case 128: return launch_b<128>(c, a, st);
        case 512: return dudf_launch_sweep_wide(c, a, st);
        default: return DUDF_E_UNSUPPORTED;
    }
}

#if DUDF_FX_CHECK
// debug build only (not part of the C ABI): granules the fixed-point packers would have wrapped since the last reset — [0] S/Q/A/Z, [1] C.
// The packers that count are the sweeps' tails, so the counters live in this unit and in dudf_sweep_wide.hip: build both with the flag.
int dudf_fx_read_wide(unsigned* out2, int reset);
extern "C" int dudf_dbg_fx_violations(unsigned* out2, int reset) {
    out2[0] = out2[1] = 0u;
    const int e = dudf_fx_read(out2, reset);
    return e ? e : dudf_fx_read_wide(out2, reset);
}
#endif
