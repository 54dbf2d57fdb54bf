// 512-wide layers (BASELINE.json configs[2]: SIREN 8x512), plain columns, training variants, on the 16-bit matrix cores
// (operand split, weight image and shared helpers: dudf_sweep16.h).
// The scheme of dudf_sweep_bf16.hip keeps this layer's AND the previous layer's accumulators in registers (2 x NT x 4): at H = 512 that
// is 256 registers before anything else, i.e. one wave per SIMD and 64-column workgroups, which the weight stream cannot
// feed.  Here a wave keeps only THIS layer's 32 accumulator tiles (128 registers, two waves per SIMD, 128-column
// workgroups as there) and the previous layer's outputs travel through the stash arrays the sweep writes anyway:
//   * when a layer's accumulators are final its elementwise tails run in one burst (same `epilogue` as everywhere: bias,
//     sin/cos or adjoint formulas, stash stores) — the post-tail value of every tile is exactly what one of those stores
//     leaves behind (forward: h_l in S; reverse: q_l in Q; adjoint forward: A_l; adjoint reverse: zbar_l in Z);
//   * the next layer reads its B operand back, one k-block (two 16-byte loads per lane) ahead of its use — this wave's
//     own 2 KB per column, written a moment ago — splits it into the three bf16 pieces, and uses it for the 32 output
//     tiles in two half-steps of 16 tiles: a weight chunk stays 48 KiB ([k-block][half]: the image of a k-block is
//     [tile][piece], so a half is contiguous) and the three-buffer LDS-DMA stream is the one of that scheme;
//   * the read-back loads are inline asm like the DMA: inside the k-loop the compiler sees no vector-memory operation,
//     every wait is hand-counted (derivation at the waits); around a tail burst everything is drained once per layer.
// Cost against the register-resident scheme: one more stash unit READ per layer and sweep (largely served by L2 / the
// Infinity Cache: it is the unit just written), and the burst is not overlapped with this wave's own MFMAs.
#include "dudf_sweep16.h"

namespace {

// kJetLane (dudf_sweep_common.h) keeps the linkage it has in dudf_sweep_bf16.hip, the unit these kernels were compiled in before: there
// the set_scale lambda of sweep_tile_b reads the table, and a lambda's use makes hipcc export a unit-local __constant__ and address it
// through the GOT.  Without this use the two jet kernels (SW = 8) address it pc-relative, and their prologue and register numbering
// move (tools/asm_diff.py); dropping it is a change to measure, not part of a move.
__device__ __forceinline__ unsigned jet_lane_linkage(int i) { return [&] { return kJetLane[i & 15]; }(); }

// which stash array carries the post-tail values of sweep SW to the next layer.  Where the tail does not store them itself
// (queries: the reverse sweep without its training stores, the jets) the kernel stores them into S, which no later tail of
// the same sweep reads.
template <int SW, int FL>
__device__ __forceinline__ const float* wide_in(const SweepArgs& a) {
    constexpr int BS = base_of(SW);
    if constexpr (BS == SWEEP_FWD) return a.S;
    else if constexpr (BS == SWEEP_REV) return (FL & 1) ? a.Q : a.S;
    else if constexpr (BS == SWEEP_ADJ_FWD) return a.A;
    else return a.Z;
}
template <int SW, int FL>
constexpr bool wide_relay_store() { return (base_of(SW) == SWEEP_REV && !(FL & 1)) || SW == SWEEP_FWD_J; }

template <int SP>
struct GeoWT {
    static constexpr int NPC = SP ? 2 : 3;              // pieces per operand (fp16 hi | lo, or bf16 h | m | l)
    static constexpr int H = 512, NT = 32, NKB = 16, FRAG = 1024;
    static constexpr int HALFT = 16;                    // tiles per half-step
    static constexpr int CHUNKB = HALFT * NPC * FRAG;   // 48 (32) KiB: one (k-block, half) of a matrix
    static constexpr int IMGB = NKB * 2 * CHUNKB;       // one matrix (= GeoB<512, SP>::IMGB)
    static constexpr int NDMA = HALFT * NPC / NWB;      // 6 (4) LDS-DMA wave-instructions per wave and chunk
    static constexpr int NTHR = 64 * NWB;
};
using GeoW = GeoWT<0>;

// SP = 1: fp16x3 (see GeoB).  The B operand of a layer is read back from the stash AFTER the whole previous layer has been
// written, so its per-column scale is exact here: 2^15 over the column's largest |output| of the tail burst.
// P24 (0 or 6): R, E as 24-bit floats and C as 24-bit fixed point, tile-major (dudf_internal.h) — the arrays that are NOT the relay.
template <int SW, int FL, int SP = 0, int P24 = 0>
__device__ __forceinline__ void sweep_tile_w(const SweepArgs& a, const int g_first, const int nact, char* lds, unsigned& gc) {
    static_assert(P24 == 0 || (P24 == 6 && SP != 0 && !is_jet(SW)), "24-bit stash arrays in the 512-wide kernel: R, E, C of the fp16x3 training variants");
    using G = GeoWT<SP>;
    constexpr int H = G::H;
    constexpr int NPC = G::NPC;
    constexpr int BS = base_of(SW);
    constexpr bool HS = is_hess(SW);                   // Hessian quads / jets: the tails couple lanes (dudf_sweep_common.h)
    constexpr bool kColScale = SP != 0 && SW != SWEEP_FWD;   // (the quads' forward tangents are not bounded by 1)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, q = lane >> 4;
    const bool isv = !HS || (is_jet(SW) ? li == 0 : (lane & 3) == 0);
    const int nhid = a.L - 1;
    constexpr bool kFwdDir = fwd_dir<SW>();
    const int64_t p = (int64_t)(g_first + wave) * 16 + li;
    auto image = [&](int j) -> const char* { return sweep_image<SW, G::IMGB, SP>(a, nhid, j); };
    auto unscale_of = [&](int j) -> float { return sweep_unscale<SW>(a, nhid, j); };
    float unscale = 1.f, sb = 1.f, inv_sb = 1.f;        // accumulators -> true values | scale of the B operand being read back
    auto in_layer = [&](int j) -> int { return sweep_in_layer<SW>(a, j); };
    auto bias_ptr = [&](int layer) -> const float* {
        return a.b1s + (size_t)layer * H;              // [L][H] biases as packed (row 0 = rho b_1)
    };
    auto stash_base = [&](int layer, int T) -> int64_t { return sweep_stash_base(a, layer, T); };
    const unsigned vo = (unsigned)(((int64_t)q * a.np + p) * 16);
    const LaneOff vl(vo, (is_hess(SW) && !is_jet(SW)) ? (unsigned)(((int64_t)q * a.np + (p >> 2)) * 16) : vo,   // C: one copy per quad
                     P24 ? (unsigned)(((p >> 4) * 64 + lane) * 12) : 0u,                                          // 24-bit tile-major arrays
                     !P24 ? 0u : (is_hess(SW) && !is_jet(SW)) ? (unsigned)(((p >> 6) * 64 + 16 * q + ((p >> 2) & 15)) * 12)
                                                              : (unsigned)(((p >> 4) * 64 + lane) * 12));
    const int total2 = nhid * G::NKB * 2;
    auto chunk_src = [&](int c2) -> const char* {       // c2 = (matrix, k-block, half), wave-uniform
        const int j = c2 / (G::NKB * 2);
        return image(j) + (size_t)(c2 - j * G::NKB * 2) * G::CHUNKB;
    };
    auto dma = [&](int c2, unsigned buf) {
        // GeoB<256, SP> has the same chunk geometry (16 tiles x NPC pieces): reuse its issue code
        dma_issue<256, SP>(chunk_src(c2), (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds + buf * G::CHUNKB,
                       (unsigned)lane * 16u, wave);
    };
    __syncthreads();                                   // every wave is past its last LDS read of the previous pass
    dma(0, gc);
    dma(1, (gc + 1) % 3);
    if (wave >= nact) {                                // idle waves of a partial pass: same DMA pieces, same barriers
        dma_wait_b<0>();
        __syncthreads();
        for (int j = 0; j < nhid; ++j) {
            for (int hs = 0; hs < G::NKB * 2; ++hs) {
                const int c2 = j * G::NKB * 2 + hs;
                const bool more = c2 + 2 < total2;
                if (more) dma(c2 + 2, (gc + 2) % 3);
                gc = (gc + 1) % 3;
                if (more) dma_wait_b<G::NDMA>(); else dma_wait_b<0>();
                __syncthreads();
            }
            dma_wait_b<0>();
            __syncthreads();                           // the barrier behind the active waves' tail burst
        }
        return;
    }

    f32x4 acc[G::NT];
    float part = 0.f;                                  // forward: y partial sums; reverse: df/dx accumulator
    f32x4 accg = {0, 0, 0, 0};
    // ---- the elementwise tails of all 32 tiles of `layer` (operands one pair ahead), stash stores, output stage ----
    constexpr int kRow = amax_row<SW, FL>();
    unsigned* lds_amax = reinterpret_cast<unsigned*>(lds + 3 * G::CHUNKB);
    auto tail_burst = [&](int layer, bool last) {
        TailTrack tmax;
        // operand ring: the stash operands of tile T + PD are requested when tile T has been consumed.  One tile of tail is
        // ~100 instructions, an HBM round trip ~2 us: with the operands only one tile ahead the burst waited for memory at
        // every tile (it took about as long as the layer's whole k-loop); the forward sweep only reads its bias (cached).
        // (three-operand tails — the quads' adjoint sweeps — get a ring of four: 128 accumulator registers leave no more)
        constexpr int PD = (BS == SWEEP_FWD) ? 2 : ((SW == SWEEP_ADJ_FWD_H || SW == SWEEP_ADJ_REV_H) ? 4 : 8);
        f32x4 o1[PD], o2[PD], o3[PD], bs[PD];
        auto ld = [&](int T, int s) {
            epilogue_loads<SW, FL, P24>(a, stash_base(layer, T), vl, o1[s], o2[s], o3[s]);
            if constexpr (BS == SWEEP_FWD) bs[s] = *reinterpret_cast<const f32x4*>(bias_ptr(layer) + 16 * T + 4 * q);
        };
        float cmax = 0.f;                              // fp16x3: largest |output| of this lane's rows of the column
#pragma unroll
        for (int T = 0; T < PD; ++T) ld(T, T);
        // (two halves of 16 tiles, each its own fully unrolled loop: as ONE loop of 32 the larger tails — the quads' adjoint forward
        //  sweep with 24-bit arrays — exceed hipcc's size limit for a forced unroll, and the rolled loop indexes acc[] dynamically)
        //  The jets' tail is too large even so; their loop stays the single rolled one it has been since round 3.)
        auto burst_range = [&](auto t0c, auto t1c) {
        constexpr int T0 = decltype(t0c)::value, T1 = decltype(t1c)::value;
#pragma unroll
        for (int T = T0; T < T1; ++T) {
            const int s = T % PD;
            f32x4 z = acc[T];
            const f32x4 zero4 = {0, 0, 0, 0};
            if constexpr (SP != 0 && SW == SWEEP_FWD) z = __builtin_elementwise_fma(z, f32x4{unscale, unscale, unscale, unscale}, bs[s]);
            else if constexpr (SW == SWEEP_FWD) z += bs[s];
            else if constexpr (BS == SWEEP_FWD) z = (SP != 0 ? z * unscale : z) + (isv ? bs[s] : zero4);   // the bias: value channel only
            else if constexpr (SP != 0) z *= unscale;
            // (RL: the array the next layer reads its operand back from keeps the default cache policy)
            const f32x4 e = epilogue<SW, FL, false, P24, true>(a, z, o1[s], o2[s], o3[s], stash_base(layer, T), vl, isv, tmax);
            if constexpr (wide_relay_store<SW, FL>()) DUDF_ST_CACHED(a.S, stash_base(layer, T), vo, e);
            if constexpr (kColScale) dudf_track(cmax, e);
            if (T + PD < G::NT) ld(T + PD, s);
            if (last) {
                // (own copy of the output stage of dudf_sweep16.h: through it nine kernels of this unit changed and the adjoint forward
                //  sweep of 8x512 took 1.8709 ms (median of three) against the parent's 1.8652 + 0.0044 of spread, profiles/HISTORY.md)
                if constexpr (BS == SWEEP_FWD) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(a.theta + a.off_wo + 16 * T + 4 * q);
                    part += e[0] * wv[0] + e[1] * wv[1] + e[2] * wv[2] + e[3] * wv[3];
                } else if constexpr (BS == SWEEP_REV) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(a.w1t16 + li * H + 16 * T + 4 * q);
#pragma unroll
                    for (int t = 0; t < 4; ++t) accg = mfma16(wv[t], e[t], accg);
                }
            }
            acc[T] = f32x4{0, 0, 0, 0};
        }
        };
        if constexpr (is_jet(SW)) {
            burst_range(std::integral_constant<int, 0>{}, std::integral_constant<int, G::NT>{});
        } else {
            burst_range(std::integral_constant<int, 0>{}, std::integral_constant<int, G::NT / 2>{});
            burst_range(std::integral_constant<int, G::NT / 2>{}, std::integral_constant<int, G::NT>{});
        }
        if constexpr (kRow >= 0) { if (layer < kMaxAmaxLayers) lds_max_wave(lds_amax + layer, tmax.t); }
        if constexpr (kColScale) {                     // the next layer's B operand = these outputs: scale the column below 2^15
            cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
            cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
            col_scale(cmax, sb, inv_sb);
        }
    };
    // ---- first layer (fp32, K = 3): pre-activations / incoming adjoints of the 32 tiles, then their tails ----
    {
        float b = 0.f, yb = 1.f;
        if constexpr (BS == SWEEP_FWD) b = (q < 3) ? a.x4[p * 4 + q] : 0.f;
        if constexpr (BS == SWEEP_ADJ_FWD) b = (q < 3) ? a.gbar[p * 4 + q] : 0.f;
        if constexpr (BS == SWEEP_ADJ_REV) yb = a.ybar[p];
        if constexpr (SW == SWEEP_REV_H) yb = isv ? 1.f : 0.f;                         // adot_L^k = 0
#pragma unroll
        for (int T = 0; T < G::NT; ++T) {
            if constexpr (kFwdDir) acc[T] = mfma16(a.w1b[(16 * T + li) * 4 + q], b, f32x4{0, 0, 0, 0});
            else acc[T] = *reinterpret_cast<const f32x4*>(a.theta + a.off_wo + 16 * T + 4 * q) * yb;
        }
        tail_burst(in_layer(0), false);
    }
    dma_wait_b<0>();                                   // chunks 0 and 1, and the burst's stores (read back below)
    __syncthreads();

    // read-back of the post-tail values of tiles 2kb, 2kb+1 of `layer`: two asm loads, scalar base + lane offset
    auto ld_in = [&](int layer, int kb, f32x4& x0, f32x4& x1) {
        const float* b0 = wide_in<SW, FL>(a) + stash_base(layer, 2 * kb);
        const float* b1 = b0 + 16 * a.np;              // next tile: 16 feature rows further (stash_base is linear in T)
        const uint64_t g0 = (uint64_t)(size_t)b0, g1 = (uint64_t)(size_t)b1;
        // (readfirstlane returns int: go through unsigned, or a low word with its top bit set sign-extends into the high word)
        const unsigned l0 = __builtin_amdgcn_readfirstlane((unsigned)g0), h0 = __builtin_amdgcn_readfirstlane((unsigned)(g0 >> 32));
        const unsigned l1 = __builtin_amdgcn_readfirstlane((unsigned)g1), h1 = __builtin_amdgcn_readfirstlane((unsigned)(g1 >> 32));
        const uint64_t s0 = ((uint64_t)h0 << 32) | l0, s1 = ((uint64_t)h1 << 32) | l1;
        asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %4"
                     : "=&v"(x0), "=&v"(x1) : "v"(vo), "s"(s0), "s"(s1) : "memory");
    };
    u32x4 bq[NPC];                                     // B operand of the current k-block
    for (int j = 0; j < nhid; ++j) {
        const int lin = in_layer(j);
        if constexpr (SP != 0) unscale = unscale_of(j) * inv_sb;     // what turns THIS matrix's accumulators into true values
        // read-back registers: `xa` carries the even k-blocks, `xb` the odd ones — the loop is unrolled by two so that a set
        // is never copied while its asm loads are in flight (a rolled loop would rotate them with v_mov at the back edge)
        f32x4 xa0, xa1, xb0, xb1;
        ld_in(lin, 0, xa0, xa1);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xa0), "+v"(xa1));      // k-block 0: nothing to overlap it with yet
        auto kstep = [&](int kb, f32x4& c0, f32x4& c1, f32x4& n0, f32x4& n1, auto steady) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c2 = (j * G::NKB + kb) * 2 + h;
                const bool more = decltype(steady)::value || c2 + 2 < total2;    // compile-time in the steady loop: one basic block
                if (h == 0) {
                    // the read-back of this k-block was issued one k-block ago; younger than it: the 6 DMA pieces of the
                    // half-step in between
                    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(c0), "+v"(c1) : "n"(G::NDMA));
                    if constexpr (kColScale) split8h(c0 * sb, c1 * sb, bq[0], bq[1]);
                    else if constexpr (SP != 0) split8h(c0, c1, bq[0], bq[1]);
                    else split8(c0, c1, bq[0], bq[1], bq[2]);
                }
                if (more) dma(c2 + 2, (gc + 2) % 3);
                if (h == 0) ld_in(lin, kb + 1 < G::NKB ? kb + 1 : kb, n0, n1);   // the last one re-reads its own: uniform counts
                __builtin_amdgcn_sched_barrier(0);
                const char* bp = lds + gc * G::CHUNKB + lane * 16;
                auto frag = [&](int T, int pc) -> u32x4 {
                    return *reinterpret_cast<const u32x4*>(bp + (T * NPC + pc) * G::FRAG);
                };
                u32x4 an[2][NPC];
#pragma unroll
                for (int T = 0; T < 2; ++T)
#pragma unroll
                    for (int pc = 0; pc < NPC; ++pc) an[T][pc] = frag(T, pc);
#pragma unroll
                for (int T = 0; T < G::HALFT; ++T) {
                    u32x4 af[NPC];
#pragma unroll
                    for (int pc = 0; pc < NPC; ++pc) af[pc] = an[T & 1][pc];
                    if (T + 2 < G::HALFT) {
#pragma unroll
                        for (int pc = 0; pc < NPC; ++pc) an[T & 1][pc] = frag(T + 2, pc);
                        __builtin_amdgcn_sched_barrier(0x76);
                    }
                    f32x4 cc = acc[G::HALFT * h + T];
                    mma_products<SP, 1, NPC>(&af, bq, &cc);
                    acc[G::HALFT * h + T] = cc;
                }
                gc = (gc + 1) % 3;
                // chunk c2+1 has landed.  Issued after its DMA: h == 0: [this step: NDMA pieces + 2 read-back]; h == 1: [previous
                // step: 2 read-back] + [this step: NDMA pieces]  ->  NDMA + 2 younger operations either way
                if (more) dma_wait_b<G::NDMA + 2>(); else dma_wait_b<0>();
                __syncthreads();
            }
        };
        const int kb_steady = (j + 1 == nhid) ? G::NKB - 2 : G::NKB;   // the stream's last two half-chunks have no successor
#pragma unroll 1                                        // 384 MFMAs per iteration: the body stays inside the instruction cache
        for (int kb = 0; kb < kb_steady; kb += 2) {
            kstep(kb, xa0, xa1, xb0, xb1, std::true_type{});
            kstep(kb + 1, xb0, xb1, xa0, xa1, std::true_type{});
        }
        if (j + 1 == nhid) {
            kstep(G::NKB - 2, xa0, xa1, xb0, xb1, std::false_type{});
            kstep(G::NKB - 1, xb0, xb1, xa0, xa1, std::false_type{});
        }
        // the last k-block's (dummy) read-back is still in flight and nothing will consume it: keep its registers until it
        // has landed, or hipcc hands them to the burst below while the load is still writing them
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xa0), "+v"(xa1), "+v"(xb0), "+v"(xb1));
        tail_burst(in_layer(j + 1), j + 1 == nhid);
        dma_wait_b<0>();
        __syncthreads();
    }
    if constexpr (BS == SWEEP_FWD) {
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (isv) part += a.theta[a.off_bo];             // tangent / jet columns are derivatives: no constant term
        if (q == 0) a.y[p] = part;
    } else if constexpr (BS == SWEEP_REV) {
        if (q == 0) *reinterpret_cast<f32x4*>(a.g + p * 4) = f32x4{accg[0], accg[1], accg[2], 0.f};
    }
}

template <int SW, int FL, int SP, int P24 = 0>
__device__ __forceinline__ void sweep_w_body(const SweepArgs& a) {
    extern __shared__ __attribute__((aligned(16))) char lds_w[];
    unsigned gc = 0;
    const bool clk_on = a.clk != nullptr && blockIdx.x == 0;
    const unsigned long long clk_t0 = clk_on ? __builtin_amdgcn_s_memtime() : 0ull, clk_r0 = clk_on ? __builtin_amdgcn_s_memrealtime() : 0ull;
    constexpr int kRow = amax_row<SW, FL>();
    unsigned* lds_amax = reinterpret_cast<unsigned*>(lds_w + 3 * GeoWT<SP>::CHUNKB);
    if constexpr (kRow >= 0) { if (threadIdx.x < kMaxAmaxLayers) lds_amax[threadIdx.x] = 0u; }
    // (measured and dropped: odd workgroups starting half a layer late, so that one half of the chip is in its compute phase
    //  — the k-loop — while the other is in its memory phase — the tail burst: +1.3 %)
    const int ng = a.ntiles * (TILE / 16), gbase = a.tile0 * (TILE / 16);
    const int g0 = (int)((int64_t)blockIdx.x * ng / gridDim.x), g1 = (int)((int64_t)(blockIdx.x + 1) * ng / gridDim.x);
    for (int g = g0; g < g1; g += NWB)
        sweep_tile_w<SW, FL, SP, P24>(a, gbase + g, (g1 - g < NWB) ? g1 - g : NWB, lds_w, gc);
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
template <int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_w_kernel(SweepArgs a) { sweep_w_body<SW, FL, 0>(a); }
template <int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_w16_kernel(SweepArgs a) { sweep_w_body<SW, FL, 1>(a); }
// ... with R, E, C at 24 bits (stash mask 6: the training variants of a default training workspace)
template <int SW, int FL>
__global__ __launch_bounds__(64 * NWB) void sweep_w16r_kernel(SweepArgs a) { sweep_w_body<SW, FL, 1, 6>(a); }

static_assert(dudf_wide_chunk_bytes(3) == GeoWT<0>::CHUNKB && dudf_wide_chunk_bytes(2) == GeoWT<1>::CHUNKB, "dudf_variants.h: LDS sizes");
int launch_w(const SweepChoice& c, const SweepArgs& a, hipStream_t st) {
    if (a.ntiles <= 0) return 0;
    const int ntb = (a.ntiles * TILE + TILEB - 1) / TILEB;
    const dim3 grid(ntb < 256 ? ntb : 256), block(GeoW::NTHR);
    return dudf_with_variant(kWideVariants, c.sw, c.fl, [&](auto i) {
        constexpr DudfVariant v = kWideVariants[decltype(i)::value];
        if (c.family == DUDF_FAM_W) return dudf_launch_kernel<&sweep_w_kernel<v.sw, v.fl>>(grid, block, c.lds, c.lds_max, st, a);
        if (c.family == DUDF_FAM_W16) return dudf_launch_kernel<&sweep_w16_kernel<v.sw, v.fl>>(grid, block, c.lds, c.lds_max, st, a);
        if constexpr (v.p24 != 0) {
            if (c.family == DUDF_FAM_W16R) return dudf_launch_kernel<&sweep_w16r_kernel<v.sw, v.fl>>(grid, block, c.lds, c.lds_max, st, a);
        }
        return (int)DUDF_E_UNSUPPORTED;
    });
}

}  // namespace

int dudf_launch_sweep_wide(const SweepChoice& c, const SweepArgs& a, hipStream_t st) { return launch_w(c, a, st); }

#if DUDF_FX_CHECK
// debug build only: this unit's share of dudf_dbg_fx_violations (dudf_sweep_bf16.hip)
int dudf_fx_read_wide(unsigned* out2, int reset) { return dudf_fx_read(out2, reset); }
#endif
