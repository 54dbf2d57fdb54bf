// Weight gradients of the DiffUDF training step: the part of `train_loss.backward()` (reference
// train.py:221) that contracts over POINTS.  SURVEY.md Appendix A.5:
//
//   dW_l[o][i] = sum_p  q_l[o][p] * A_{l-1}[i][p]  +  zbar_l[o][p] * s_{l-1}[i][p]        (l = 2..L)
//   db_l[o]    = sum_p  zbar_l[o][p]
//   dW_1[o][d] = sum_p  q_1[o][p] * gbar[p][d]  +  zbar_1[o][p] * x[p][d] ;  db_1 = sum_p zbar_1
//   dW_out[f]  = sum_p  A_L[f][p] + ybar[p] * s_L[f][p] ;                     db_out = sum_p ybar
//
// The sweeps leave q, A, zbar, s in HBM as [layer][feature/4][point][4] (dudf_internal.h).  That is
// the K-major layout a GEMM whose K dimension is the point index wants, so the hidden layers are one
// v_mfma_f32_32x32x2_f32 GEMM per layer (M = N = H, K = 2*n points) split over point ranges:
// a workgroup owns the whole HxH tile of one layer for a range of points, stages 32 points of the two
// operands through LDS per step ([fq][33][4] floats: the 33 makes the per-feature b32 reads
// conflict-free), and adds its partial tile into dtheta with float atomics at the end (each atomic
// wave-instruction is two 128-byte row segments — the full-rate shape; 256 KB per workgroup).
// The bias gradient rides along on the VALU beside the MFMAs: running row sums of zbar over the value columns
// (every column on the plain range, channel 0 of each quad on the Hessian range; padding columns hold zeros).
// The two thin layers (3 inputs / 1 output) are a bandwidth-bound VALU reduction.
#include "dudf_internal.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {

template <int H> struct WG;
template <> struct WG<256> { static constexpr int WO = 4, WI = 2, MT = 2, NTL = 4; };
template <> struct WG<128> { static constexpr int WO = 4, WI = 2, MT = 1, NTL = 2; };
template <> struct WG<64>  { static constexpr int WO = 2, WI = 2, MT = 1, NTL = 1; };
template <> struct WG<32>  { static constexpr int WO = 1, WI = 1, MT = 1, NTL = 1; };

constexpr int KT = 32;          // points per LDS stage
constexpr int KTP = 33;         // padded

struct WgradArgs {
    const float *Q, *A, *Z, *S;         // stash arrays
    int64_t ncol_h;                     // columns [0, ncol_h) are Hessian quads: only channel 0 (col % 4 == 0) carries the bias
    float* dtheta;
    int64_t np, stash_layer, off_hid, hid_stride;
    int steps_total;                    // np / KT
    int L;
    int have_g;                         // 0: loss without df/dx terms (loss_s2) -> only the zbar*s pair
    int j0, nj;                         // hidden matrices [j0, j0 + nj) of this launch (matrix j = layer l = j + 2); grid.x = nj
    int Hs;                             // real layer width; the kernels' template H is the output TILE (<= 256):
                                        // blockIdx.z walks the (Hs/H)^2 tiles of a wider layer
    int remap_nsplit;                   // > 0: 1-D grid, the output tiles of one (layer, column split) share an XCD (see wgrad_pipeline)
    unsigned long long* clk;            // profiling: (shader clock, 100 MHz reference) ticks of workgroup (0,0,0), or nullptr
    const unsigned* amax;               // [4][L] bit patterns of max |q_l|, |A_l|, |zbar_l| over all columns (fp16x3 kernel)
    const float *fxS, *fxQ, *fxA, *fxZ; // 24-bit tile-major operands (DudfLayout::p24 bit 0): [L][np] — per layer and column the power of two 2^E of that array's values (dudf_sweep_common.h fx24_pack)
};

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// What the three GEMM bodies share.  A workgroup (bx, by, bz) owns output tile bz of hidden matrix j = bx + j0 for the
// stages [s0, s1) of `steps` (column split by of nsplit) and walks them as nit (stage, pair) iterations:
// pair 0: X = q_l (layer index j+1), Y = A_{l-1} (index j);  pair 1: X = zbar_l, Y = s_{l-1}
struct WgTile {
    int j, s0, s1, o_off, i_off, have_g, nit;
    const float *X0, *X1, *Y0, *Y1;
    // (Idx: blockIdx's unsigned as it is, or the int of a remapped grid — the divisions below are those of that type)
    template <class Idx>
    __device__ __forceinline__ WgTile(const WgradArgs& a, int H, Idx bx, Idx by, Idx bz, int nsplit, int steps, int64_t lstride) {
        j = bx + a.j0;                                  // hidden matrix index: layer l = j + 2
        s0 = (int)((int64_t)steps * by / nsplit);
        s1 = (int)((int64_t)steps * (by + 1) / nsplit);
        const int tz = a.Hs / H;                        // output tiles per side
        o_off = (bz / tz) * H; i_off = (bz % tz) * H;
        const int64_t xrow = (int64_t)(o_off / 4) * a.np * 4, yrow = (int64_t)(i_off / 4) * a.np * 4;
        X0 = a.Q + (int64_t)(j + 1) * lstride + xrow;
        X1 = a.Z + (int64_t)(j + 1) * lstride + xrow;
        Y0 = a.A + (int64_t)j * lstride + yrow;
        Y1 = a.S + (int64_t)j * lstride + yrow;
        have_g = a.have_g;
        nit = (have_g ? 2 : 1) * (s1 - s0);
    }
    __device__ __forceinline__ int pair_of(int it) const { return have_g ? (it & 1) : 1; }
    __device__ __forceinline__ int step_of(int it) const { return s0 + (have_g ? (it >> 1) : it); }
    // this tile's corner of the weight gradient and its slice of the bias gradient
    __device__ __forceinline__ float* dW(const WgradArgs& a) const { return a.dtheta + a.off_hid + (int64_t)j * a.hid_stride + (int64_t)o_off * a.Hs + i_off; }
    __device__ __forceinline__ float* dB(const WgradArgs& a) const { return a.dtheta + a.off_hid + (int64_t)j * a.hid_stride + (int64_t)a.Hs * a.Hs + o_off; }
};
template <int M, int N>
__device__ __forceinline__ void wg_zero(f32x16 (&acc)[M][N]) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
}
// wave (wo, wi) adds its accumulators (times `scale`: a literal 1 folds away) into the tile of dtheta
// D layout 32x32: col = lane&31 (input index i), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) (output index o)
template <int H>
__device__ __forceinline__ void wg_add_tile(const WgradArgs& a, float* dW, int wo, int wi,
                                            const f32x16 (&acc)[WG<H>::MT][WG<H>::NTL], float scale = 1.f) {
    using W = WG<H>;
    const int l32 = threadIdx.x & 31, hh = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int m = 0; m < W::MT; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = (wo * W::MT + m) * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
#pragma unroll
            for (int n = 0; n < W::NTL; ++n) {
                const int i = (wi * W::NTL + n) * 32 + l32;
                atomicAdd(dW + (int64_t)o * a.Hs + i, acc[m][n][e] * scale);
            }
        }
}

template <int H>
__device__ __forceinline__ void wgrad_hidden_body(const WgradArgs& a) {
    using W = WG<H>;
    constexpr int NTHR = 64 * W::WO * W::WI;
    constexpr int FQ = H / 4;                       // feature quads per operand
    constexpr int TILE = FQ * KTP * 4;              // floats per staged operand
    constexpr int F4 = FQ * KT;                     // float4 per operand per stage
    constexpr int NLD = (F4 + NTHR - 1) / NTHR;
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [2 buffers][X tile | Y tile]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wo = wave / W::WI, wi = wave % W::WI;
    const int l32 = lane & 31, hh = lane >> 5;
    const WgTile t(a, H, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, a.steps_total, a.stash_layer);

    f32x16 acc[W::MT][W::NTL];
    float bsum[W::MT] = {};                         // bias gradient: running row sums of zbar (VALU, beside the MFMAs)
    wg_zero(acc);

    f32x4 rx[NLD], ry[NLD];
    auto issue = [&](int pair, int step) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int f = tid + NTHR * u;
            if (F4 % NTHR == 0 || f < F4) {
                const int fq = f / KT, pt = f % KT;
                const int64_t off = ((int64_t)fq * a.np + (int64_t)step * KT + pt) * 4;
                rx[u] = *reinterpret_cast<const f32x4*>((pair ? t.X1 : t.X0) + off);
                ry[u] = *reinterpret_cast<const f32x4*>((pair ? t.Y1 : t.Y0) + off);
            }
        }
    };
    auto commit = [&](float* buf) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int f = tid + NTHR * u;
            if (F4 % NTHR == 0 || f < F4) {
                const int fq = f / KT, pt = f % KT;
                *reinterpret_cast<f32x4*>(buf + (fq * KTP + pt) * 4) = rx[u];
                *reinterpret_cast<f32x4*>(buf + TILE + (fq * KTP + pt) * 4) = ry[u];
            }
        }
    };

    if (t.nit > 0) {
        issue(t.pair_of(0), t.step_of(0));
        commit(lds);
    }
    __syncthreads();
    for (int it = 0; it < t.nit; ++it) {
        const float* buf = lds + (it & 1) * 2 * TILE;
        if (it + 1 < t.nit) issue(t.pair_of(it + 1), t.step_of(it + 1));      // next stage: global -> registers
        // bias mask of this stage's columns: k index 2*kk+hh is a value column always (plain range) or when
        // (2*kk+hh) % 4 == 0 (Hessian range: stages never straddle the two ranges)
        const float bflag = (t.pair_of(it) == 1 && wi == 0 && t.i_off == 0) ? 1.f : 0.f;
        const bool hstage = (int64_t)t.step_of(it) * KT < a.ncol_h;
        const float f_even = hstage ? (hh == 0 ? bflag : 0.f) : bflag;
        const float f_odd = hstage ? 0.f : bflag;
        const float* xa[W::MT];
        const float* yb[W::NTL];
#pragma unroll
        for (int m = 0; m < W::MT; ++m) {
            const int feat = (wo * W::MT + m) * 32 + l32;
            xa[m] = buf + ((feat >> 2) * KTP) * 4 + (feat & 3);
        }
#pragma unroll
        for (int n = 0; n < W::NTL; ++n) {
            const int feat = (wi * W::NTL + n) * 32 + l32;
            yb[n] = buf + TILE + ((feat >> 2) * KTP) * 4 + (feat & 3);
        }
#pragma unroll
        for (int kk = 0; kk < KT / 2; ++kk) {
            const int pt = 2 * kk + hh;             // MFMA k index = lane>>5
            float av[W::MT], bv[W::NTL];
#pragma unroll
            for (int m = 0; m < W::MT; ++m) av[m] = xa[m][pt * 4];
#pragma unroll
            for (int n = 0; n < W::NTL; ++n) bv[n] = yb[n][pt * 4];
#pragma unroll
            for (int m = 0; m < W::MT; ++m) {
#pragma unroll
                for (int n = 0; n < W::NTL; ++n) acc[m][n] = mfma32(av[m], bv[n], acc[m][n]);
                bsum[m] = fmaf(av[m], (kk & 1) ? f_odd : f_even, bsum[m]);
            }
        }
        // the other buffer was last read in iteration it-1 and every wave is past that iteration's barrier
        if (it + 1 < t.nit) commit(lds + ((it + 1) & 1) * 2 * TILE);
        __syncthreads();
    }

    float* dW = t.dW(a);
    float* dB = t.dB(a);
    if (t.nit > 0) {
        wg_add_tile<H>(a, dW, wo, wi, acc);
#pragma unroll
        for (int m = 0; m < W::MT; ++m) {
            // lane (l32, hh) summed zbar[feature l32] over the points of parity hh
            const float tot = bsum[m] + __shfl_xor(bsum[m], 32);
            if (wi == 0 && hh == 0 && t.i_off == 0) atomicAdd(dB + (wo * W::MT + m) * 32 + l32, tot);
        }
    }
}
template <int H>
__global__ __launch_bounds__(64 * WG<H>::WO * WG<H>::WI) DUDF_NO_PK void wgrad_hidden_kernel(WgradArgs a) { wgrad_hidden_body<H>(a); }   // no packed fp32: see dudf_internal.h

// ---- the same GEMM on the bf16 matrix cores, at fp32 accuracy ("bf16x6") ---------------------------------------------
// Every fp32 operand is split EXACTLY into three bf16 pieces v = h + m + l (8+8+8 significand bits); a product a*b is
// the six piece products with combined order <= 2 (hh, hm, mh, hl, lh, mm), each exact in the MFMA and accumulated in
// fp32; the dropped ones (ml, lm, ll) are <= 2^-24 relative, the size of one fp32 rounding.  Six
// v_mfma_f32_32x32x16_bf16 (32 cycles, K = 16) replace eight v_mfma_f32_32x32x2_f32 (64 cycles, K = 2) per 16 points:
// 2.67x less matrix-pipe time for the same 183 GFLOP.  The split (5.5 VALU ops per element, only of the fragments a
// wave consumes) runs beside the MFMAs.  tests/test_hip_parity.py holds the result to the SAME tolerances as fp32.
__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

struct Split3 { bf16x8 h, m, l; };

// 8 consecutive columns c0..c0+7 of one feature out of the swizzled [fq][16][4] image (column c sits at slot c ^ swz)
// -> three bf16 fragments, worked on as packed pairs (3 cvt_pk + 4 bit ops + 2 packed subtracts per pair), + the
// masked row sum for the bias gradient
__device__ __forceinline__ Split3 load_split_swz(const float* row, int c0, int swz, float& sum, float f_other) {
    u32x4 hp, mp, lp;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 v = {row[((c0 + 2 * i) ^ swz) * 4], row[((c0 + 2 * i + 1) ^ swz) * 4]};
        const unsigned h = cvt_pk(v);
        const f32x2 r1 = v - unpack(h);
        const unsigned m = cvt_pk(r1);
        const f32x2 r2 = r1 - unpack(m);
        hp[i] = h; mp[i] = m; lp[i] = cvt_pk(r2);
        acc += ((i & 1) == 0 ? v.x : v.x * f_other) + v.y * f_other;     // Hessian range: only columns % 4 == 0 count
    }
    sum = acc;
    Split3 r;
    r.h = __builtin_bit_cast(bf16x8, hp); r.m = __builtin_bit_cast(bf16x8, mp); r.l = __builtin_bit_cast(bf16x8, lp);
    return r;
}

// Staging for this kernel: LDS-DMA (inline asm, see dudf_sweep.hip for why) into a 4-deep ring of 16-column stages.
// The image of one operand is [feature quad][16 columns][4 features] WITHOUT padding (a DMA wave-instruction writes
// 1 KiB linearly); bank conflicts of the per-feature b32 reads are removed by storing column c of quad fq at slot
// c ^ (fq & 7) — applied through the per-lane SOURCE address of the DMA and again on the read.  Three stages are in
// flight behind a counted vmcnt, because at bf16 rates a stage is consumed in ~1.5 us — less than an HBM round trip.
constexpr int KB = 16;          // columns per stage of the bf16 kernel
constexpr int NRING = 4;

template <int H>
__device__ __forceinline__ void wgrad_hidden_bf16_body(const WgradArgs& a) {
    using W = WG<H>;
    constexpr int NW_ = W::WO * W::WI;
    constexpr int FQ = H / 4;
    constexpr int OPER = FQ * KB * 4;                       // floats per operand image
    constexpr int STAGE = 2 * OPER;                         // X image | Y image
    constexpr int PIECES = (FQ * KB) / 64;                  // 1 KiB DMA pieces per operand image
    static_assert(PIECES % NW_ == 0, "every wave stages the same number of pieces");
    constexpr int PPW = PIECES / NW_;                       // pieces per wave and operand
    constexpr int PER_WAVE = 2 * PPW;                       // DMA instructions per wave and stage
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [NRING][X image | Y image]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave / W::WI, wi = wave % W::WI;
    const int l32 = lane & 31, hh = lane >> 5;
    const WgTile t(a, H, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y, a.steps_total * (KT / KB), a.stash_layer);

    f32x16 acc[W::MT][W::NTL];
    float bsum[W::MT] = {};
    wg_zero(acc);

    // lane part of the DMA source: granule (fq_in_piece = lane/16, slot = lane%16) holds column slot ^ (fq & 7)
    auto issue = [&](int it) {
        const int pair = t.pair_of(it);
        const int64_t col0 = (int64_t)t.step_of(it) * KB;
        float* ring = lds + (it % NRING) * STAGE;
        const float* xs = pair ? t.X1 : t.X0;
        const float* ys = pair ? t.Y1 : t.Y0;
#pragma unroll
        for (int oper = 0; oper < 2; ++oper) {
#pragma unroll
            for (int v = 0; v < PPW; ++v) {
                const int piece = wave + NW_ * v;           // wave-uniform 1 KiB piece of this operand's image
                const int fq = piece * 4 + (lane >> 4);
                const int col = (lane & 15) ^ (fq & 7);
                const float* src = (oper ? ys : xs) + ((int64_t)fq * a.np + col0 + col) * 4;
                const unsigned dst = __builtin_amdgcn_readfirstlane(
                    (unsigned)(size_t)(__attribute__((address_space(3))) float*)(ring + oper * OPER + piece * 256));
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\t"
                             "s_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(dst) : "memory");    // nt: the stash is read once here
            }
        }
    };
    // prologue: three stages in flight
    for (int it = 0; it < NRING - 1 && it < t.nit; ++it) issue(it);
    if (t.nit > 0) {
        if (t.nit >= 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PER_WAVE) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int it = 0; it < t.nit; ++it) {
        // the ring slot of stage it+3 was read in iteration it-1; every wave is past that iteration's barrier
        if (it + NRING - 1 < t.nit) issue(it + NRING - 1);
        const float* buf = lds + (it % NRING) * STAGE;
        const float bflag = (t.pair_of(it) == 1 && wi == 0 && t.i_off == 0) ? 1.f : 0.f;
        const bool hstage = (int64_t)t.step_of(it) * KB < a.ncol_h;
        const float f_other = hstage ? 0.f : 1.f;
        const int c0 = 8 * hh;                                    // MFMA k = 8*(lane>>5) + jj -> column c0 + jj
        Split3 af[W::MT];
#pragma unroll
        for (int m = 0; m < W::MT; ++m) {
            const int feat = (wo * W::MT + m) * 32 + l32;
            float rs;
            af[m] = load_split_swz(buf + (feat >> 2) * (KB * 4) + (feat & 3), c0, (feat >> 2) & 7, rs, f_other);
            bsum[m] = fmaf(rs, bflag, bsum[m]);
        }
#pragma unroll
        for (int n = 0; n < W::NTL; ++n) {
            const int feat = (wi * W::NTL + n) * 32 + l32;
            float dummy;
            const Split3 bf = load_split_swz(buf + OPER + (feat >> 2) * (KB * 4) + (feat & 3), c0, (feat >> 2) & 7,
                                             dummy, 1.f);
#pragma unroll
            for (int m = 0; m < W::MT; ++m) {
                f32x16 c = acc[m][n];
                c = mfma_bf16(af[m].m, bf.m, c);              // smallest terms first
                c = mfma_bf16(af[m].l, bf.h, c);
                c = mfma_bf16(af[m].h, bf.l, c);
                c = mfma_bf16(af[m].m, bf.h, c);
                c = mfma_bf16(af[m].h, bf.m, c);
                c = mfma_bf16(af[m].h, bf.h, c);
                acc[m][n] = c;
            }
        }
        // stage it+1 has landed: all but the DMA pieces of the (up to) two younger stages are retired
        if (it + 1 < t.nit) {
            if (it + 3 < t.nit) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PER_WAVE) : "memory");
            else if (it + 2 < t.nit) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PER_WAVE) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }

    float* dW = t.dW(a);
    float* dB = t.dB(a);
    if (t.nit > 0) {
        wg_add_tile<H>(a, dW, wo, wi, acc);
#pragma unroll
        for (int m = 0; m < W::MT; ++m) {
            const float tot = bsum[m] + __shfl_xor(bsum[m], 32);
            if (wi == 0 && hh == 0 && t.i_off == 0) atomicAdd(dB + (wo * W::MT + m) * 32 + l32, tot);
        }
    }
}
template <int H>
__global__ __launch_bounds__(64 * WG<H>::WO * WG<H>::WI) DUDF_NO_PK void wgrad_hidden_bf16_kernel(WgradArgs a) { wgrad_hidden_bf16_body<H>(a); }   // no packed fp32: see dudf_internal.h

// ---- bf16x6 / fp16x3 with a COOPERATIVE split (256 x 256 tiles) -------------------------------------------------------
// The kernel above is bound by vector-ALU issue, not by the matrix cores: every wave splits the fragments it consumes, so
// an X element is split by 2 waves and a Y element by 4 (7.5 VALU instructions per MFMA, PMC).  Here every element is
// split ONCE: a stage (16 columns x 256 features x 2 operands = 2048 16-byte granules) is dealt out 4 granules per lane,
// loaded straight into registers (no raw copy in LDS), split, and written as 16-bit pieces into an LDS image that the
// MFMA fragments are read back from.  Two things make up a build:
//   * the PIPELINE (wgrad_pipeline), the same for all builds: progress flags in LDS instead of barriers, three register
//     sets in flight across the back edge behind hand-counted vmcnt, the hot loop of three stages, the drains, the MFMA
//     groups and the hand-over flag;
//   * the STAGER, the format a stage travels in — which granules a lane loads, how they are split, where the pieces go in
//     the image and how a fragment comes back out: RowStager (row granules, fragment-ordered image, ds_read_b128) or
//     TileStager (tile granules, [column][feature] image, ds_read_b64_tr_b16).
// There is no workgroup barrier per stage: NB = 3 or 4 images live in LDS beside per-wave progress counters (the flags, see
// wg_poll below).  A wave starts stage `it` when all eight waves have written image `it`, multiplies FIRST, and behind its
// MFMAs splits image it + 2 — two images ahead — whose register set is then refilled with the stage three further on.
// (Predecessors — two images and a barrier per stage, split slices between the MFMA groups, static wave priorities: DESIGN.md
// Appendix A has their numbers, `git log -- diffudf_amd/csrc/dudf_wgrad.hip` their code.)
// Cache policy of the staging loads: no non-temporal hint.  A lane's four loads sit 64 bytes apart, so every 128-byte line is
// touched by two different instructions.  While round 3's workspace layout had the stash 64 bytes off the line grid (fixed:
// dudf_make_layout), the hinted loads fetched 4.17 GB per launch against 2.87 GB of operands and 3.04 GB without the hint
// (profiles/r03_wgrad_nt.txt); on the aligned layout both forms fetch 2.87 GB and take the same time.
constexpr int kHandOver = 2;       // a wave hands the matrix pipe over this many MFMA groups before the end of a stage
// SP = 1: the fp16 hi/lo split ("fp16x3": products hi*hi + hi*lo + lo*hi, see dudf_sweep_bf16.hip) — half the MFMAs, two
// pieces instead of three to convert, write and read back.  fp16's range is bought with per-layer powers of two: the
// sweeps leave max |q_l|, |A_l|, |zbar_l| over all columns in `amax` (|s_l| <= 1); each operand is scaled so that its
// largest element lands below 2^15, the two pairs of a layer (q A^T and zbar s^T accumulate into the same registers) are
// brought to a common product scale 2^P, and the accumulators are multiplied by 2^-P at the end.  Elements more than 2^16
// below their tensor's maximum lose relative (not absolute) accuracy: they are fp16 subnormals, which v_cvt_pk_f16_f32
// produces and the MFMA honours (profiles/r03_f16_split_facts.txt).
__device__ __forceinline__ f32x16 mfma_f16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int dudf_exp_above(unsigned bits) {     // e with |v| < 2^e, clamped to a range that keeps every scale finite
    const int e = (int)((bits >> 23) & 255u) - 126;
    return e < -40 ? -40 : (e > 60 ? 60 : e);
}
__device__ __forceinline__ float dudf_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }

// The fp16 hi/lo pieces of four values as packed dwords.  hi = fp16(v scl) comes from the caller (the stagers round it with
// different instructions); lo = fp16(v scl - hi): the residual as ONE v_fma_mix_f32 per value (exact; reads the fp16 half in
// place and issues beside the SIMD partner's MFMAs like v_fma_f32 — tools/micro/coissue.hip).  `scl` is wave-uniform (an SGPR
// operand); the overload without it multiplies by the literal 1.0.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct F16HiLo { u32x2 hi, lo; };
__device__ __forceinline__ F16HiLo f16_pack(f16x2 h0, f16x2 h1, f32x2 r0, f32x2 r1) {
    const f16x2 l0 = __builtin_convertvector(r0, f16x2), l1 = __builtin_convertvector(r1, f16x2);
    return F16HiLo{u32x2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)},
                   u32x2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)}};
}
__device__ __forceinline__ F16HiLo f16_hi_lo(f32x2 v0, f32x2 v1, f16x2 h0, f16x2 h1, float scl) {
    f32x2 r0, r1;
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r0.x) : "v"(v0.x), "s"(scl), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r0.y) : "v"(v0.y), "s"(scl), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r1.x) : "v"(v1.x), "s"(scl), "v"(h1));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r1.y) : "v"(v1.y), "s"(scl), "v"(h1));
    return f16_pack(h0, h1, r0, r1);
}
__device__ __forceinline__ F16HiLo f16_hi_lo(f32x2 v0, f32x2 v1, f16x2 h0, f16x2 h1) {
    f32x2 r0, r1;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r0.x) : "v"(v0.x), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r0.y) : "v"(v0.y), "v"(h0));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r1.x) : "v"(v1.x), "v"(h1));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r1.y) : "v"(v1.y), "v"(h1));
    return f16_pack(h0, h1, r0, r1);
}
template <int pieceb>
__device__ __forceinline__ void put_hi_lo(char* dst, const F16HiLo& p) {       // the hi piece's image, then the lo piece's
    *reinterpret_cast<u32x2*>(dst) = p.hi;
    *reinterpret_cast<u32x2*>(dst + pieceb) = p.lo;
}
// a wave-uniform address as a scalar register pair: the base of the asm staging loads (scalar base + the lane's fixed 32-bit
// byte offset: no per-stage 64-bit address arithmetic in vector registers)
__device__ __forceinline__ uint64_t wg_uniform64(const void* p) {
    const uint64_t g0 = (uint64_t)(size_t)p;
    const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)g0), hi32 = __builtin_amdgcn_readfirstlane((unsigned)(g0 >> 32));
    return ((uint64_t)hi32 << 32) | lo32;
}

// What the two stagers share: the wave's producer operand (waves 0..3 stage X, 4..7 stage Y), its fp16x3 layer scales and
// which of the lane's values count towards the bias gradient.  A stager's interface to the pipeline:
//   NPC, PIECEB / OPERB / BUFB   pieces per operand and the bytes of a piece, an operand, an image buffer
//   RawSet, kSetLoads, drain     the registers a stage travels in, its loads, and the wait for all three sets
//   layer_stride(a)              floats per layer of the operand arrays
//   load / load_plain            stage `it` -> a register set: inline asm for the hand-counted loop, ordinary loads outside it
//   wait<N>(r)                   set r has landed; the N loads issued after it stay in flight
//   split_store(it, r, buf)      registers -> the pieces of image buffer `buf` (+ the bias sums)
//   fragA / fragB(buf, block, piece)   this lane's part of an MFMA fragment
//   flush_bias(dB)               the bias sums -> dtheta
struct StagerBase {
    using W = WG<256>;
    static constexpr int NW_ = W::WO * W::WI;
    const WgradArgs& a;
    const WgTile& t;
    char* ldsb;
    int p_oper, wo, wi;
    const float *P0, *P1;                   // this wave's operand for the (q, A) / (zbar, s) pair
    float sc0 = 1.f, sc1 = 1.f;             // fp16x3: its power of two for each pair, set by the pipeline
    float bm_plain, bm_quad;
    __device__ __forceinline__ StagerBase(const WgradArgs& a_, const WgTile& t_, char* ldsb_, int tid, int wave)
        : a(a_), t(t_), ldsb(ldsb_), p_oper(wave / (NW_ / 2)), wo(wave / W::WI), wi(wave % W::WI),
          P0(p_oper ? t_.Y0 : t_.X0), P1(p_oper ? t_.Y1 : t_.X1) {
        bm_plain = (p_oper == 0 && t.i_off == 0) ? 1.f : 0.f;           // this lane's granules count towards the bias gradient ...
        bm_quad = ((tid & 3) == 0) ? bm_plain : 0.f;            // ... on a Hessian-quad stage (the value channel: column % 4 == 0)
    }
    // once per stage: the zbar pair only, and on a Hessian-quad stage only the value channel
    // (branch-free: scalar selects times per-lane constants — a branch here would cut the hand-counted loop body into
    //  several basic blocks)
    __device__ __forceinline__ float bias_mask(int it) const {
        const float hs = ((int64_t)t.step_of(it) * KB < a.ncol_h) ? 1.f : 0.f;
        const float pf = t.pair_of(it) == 1 ? 1.f : 0.f;
        return pf * (bm_plain + hs * (bm_quad - bm_plain));
    }
    __device__ __forceinline__ float layer_scale(int it) const {
        return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(t.pair_of(it) ? sc1 : sc0)));
    }
    __device__ __forceinline__ const float* operand(int it) const { return t.pair_of(it) ? P1 : P0; }
};

// Row granules: a lane takes four columns of one feature quad of the fp32 stash rows (its four lanes read 64 contiguous bytes
// per instruction) and writes its pieces into an image laid out in MFMA-FRAGMENT order ([operand][piece][32-feature block][column half][feature]
// [8 columns]: a fragment is two lane-linear 512-byte halves, conflict-free for ds_read_b128; the halves are 528 bytes apart so
// that the 8-byte writes do not collide).  Producer lanes are dealt out so that each ds_write_b64 wave-instruction is bank-conflict
// free (a 16-lane service group spans offsets 16 a + 2 b + 4 c + 8 d dwords: fq bit 0 | column-group bit 0 | column half | fq
// bit 3); the plain (tid >> 2) order put feature quads 0/2 and 1/3 of a group on the same banks (PMC r01: 29 % of LDS cycles).
// SP = 0: three bf16 pieces; SP = 1: fp16 hi / lo.
template <int SP>
struct RowStager : StagerBase {
    static constexpr int NPC = SP ? 2 : 3;
    static constexpr int HALFB = 32 * 16 + 16;              // 32 features x 8 columns of a block, +16: the second column half
    static constexpr int BLKB = 2 * HALFB;                  //   must not sit 512 B = 0 banks after the first (ds_write_b64)
    static constexpr int PIECEB = (256 / 32) * BLKB;        // 8.25 KiB
    static constexpr int OPERB = NPC * PIECEB;              // 24 KiB (SP: 16.5)
    static constexpr int BUFB = 2 * OPERB;                  // 48 KiB (33)
    static constexpr int kSetLoads = 4;
    struct RawSet { f32x4 g0, g1, g2, g3; };                // granule j: 4 features of column 4 * cg + j
    __device__ static __forceinline__ int64_t layer_stride(const WgradArgs& a) { return a.stash_layer; }
    __device__ static __forceinline__ void drain(RawSet& r0, RawSet& r1, RawSet& r2) {      // everything in flight has landed
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(r0.g0), "+v"(r0.g1), "+v"(r0.g2), "+v"(r0.g3), "+v"(r1.g0), "+v"(r1.g1),
                     "+v"(r1.g2), "+v"(r1.g3), "+v"(r2.g0), "+v"(r2.g1), "+v"(r2.g2), "+v"(r2.g3));
    }

    int p_cg, p_fq, p_loff, c_lane;         // producer role of this lane: group of four columns, feature quad, image offset; its fragment offset
    int64_t p_goff;
    unsigned p_voff;
    f32x4 bacc = {0.f, 0.f, 0.f, 0.f};                      // bias gradient partial sums (X operand, zbar pair)
    __device__ __forceinline__ RowStager(const WgradArgs& a_, const WgTile& t_, char* ldsb_, int tid, int wave)
        : StagerBase(a_, t_, ldsb_, tid, wave) {
        const int lane = tid & 63;
        p_cg = tid & 3;
        p_fq = ((tid >> 2) & 1) | (((tid >> 4) & 3) << 1) | (((tid >> 3) & 1) << 3) | (((tid >> 6) & 3) << 4);   // conflict-free writes: see above
        // granule j of this lane = stage column p_cg + 4 j: one load instruction then reads 64 contiguous bytes per feature
        // quad (4 lanes x 16 B) and touches each 128-byte line twice instead of four times (PMC r01: 2x the ideal L2
        // requests; the loads alone held the kernel at 0.8 ms).  The image slot 4 p_cg + j therefore holds column p_cg + 4 j:
        // a permutation of the contraction index, the same for both operands, hence free.
        p_goff = ((int64_t)p_fq * a.np + p_cg) * 4;             // floats, + col0 * 4 per stage
        p_loff = p_oper * OPERB + (p_fq >> 3) * BLKB + (p_cg >> 1) * HALFB + ((p_fq & 7) * 4) * 16 + (p_cg & 1) * 8;   // + f * 16 + piece * PIECEB
        p_voff = (unsigned)(p_goff * 4);                        // (the launcher keeps FQ * np * 16 below 2^32)
        c_lane = (lane >> 5) * HALFB + (lane & 31) * 16;        // consumer role: fragment (32-feature block b, piece p) of an operand = 1 KiB, lane-linear
    }
    // Inline asm + hand-counted vmcnt (as in the sweeps): with compiler-visible loads hipcc drains ALL stages in flight
    // (vmcnt(0)) at the loop head.  A set's loads are the only vector-memory operations of the loop.
    __device__ __forceinline__ void load(int it, RawSet& r) const {
        const uint64_t sbase = wg_uniform64(operand(it) + (int64_t)t.step_of(it) * KB * 4);
        asm volatile("global_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:64\n\t"
                     "global_load_dwordx4 %2, %4, %5 offset:128\n\tglobal_load_dwordx4 %3, %4, %5 offset:192"
                     : "=&v"(r.g0), "=&v"(r.g1), "=&v"(r.g2), "=&v"(r.g3) : "v"(p_voff), "s"(sbase) : "memory");
    }
    // outside the steady-state loop (prologue, last stages: conditional loads) the loads are ordinary ones: a conditional
    // asm load makes hipcc merge "loaded" and "not loaded" values with register copies — of registers still in flight
    __device__ __forceinline__ void load_plain(int it, RawSet& r) const {
        const float* src = operand(it) + p_goff + (int64_t)t.step_of(it) * KB * 4;
        r.g0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
        r.g1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src) + 4);
        r.g2 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src) + 8);
        r.g3 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src) + 12);
    }
    template <int N>
    __device__ static __forceinline__ void wait(RawSet& r) {
        asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r.g0), "+v"(r.g1), "+v"(r.g2), "+v"(r.g3) : "n"(N));
    }
    __device__ __forceinline__ void split_slice(int it, const RawSet& r, int f, int bsel) {    // feature f of the lane's quad -> piece image buffer bsel
        char* dst = ldsb + bsel * BUFB + p_loff + 16 * f;
        // Hessian quads: only columns % 4 == 0 (the value channel) carry the bias — all four granules of the lanes
        // with p_cg == 0, none of the others
        if (f == 0) bacc += bias_mask(it) * (r.g0 + r.g1 + r.g2 + r.g3);
        const f32x2 v0 = {r.g0[f], r.g1[f]}, v1 = {r.g2[f], r.g3[f]};     // four columns of one feature -> NPC x 8 bytes
        if constexpr (SP != 0) {
            const float scl = layer_scale(it);                            // t = v 2^k -> hi = fp16(t), lo = fp16(t - hi)
            const f16x2 h0 = __builtin_convertvector(v0 * scl, f16x2), h1 = __builtin_convertvector(v1 * scl, f16x2);
            put_hi_lo<PIECEB>(dst, f16_hi_lo(v0, v1, h0, h1, scl));
        } else {
            const unsigned h0 = cvt_pk(v0), h1 = cvt_pk(v1);
            const f32x2 r0 = v0 - unpack(h0), r1 = v1 - unpack(h1);
            const unsigned m0 = cvt_pk(r0), m1 = cvt_pk(r1);
            const f32x2 q0 = r0 - unpack(m0), q1 = r1 - unpack(m1);
            const unsigned l0 = cvt_pk(q0), l1 = cvt_pk(q1);
            *reinterpret_cast<u32x2*>(dst) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(dst + PIECEB) = u32x2{m0, m1};
            *reinterpret_cast<u32x2*>(dst + 2 * PIECEB) = u32x2{l0, l1};
        }
    }
    __device__ __forceinline__ void split_store(int it, const RawSet& r, int bsel) {
#pragma unroll
        for (int f = 0; f < 4; ++f) split_slice(it, r, f, bsel);
    }
    __device__ __forceinline__ u32x4 fragA(const char* buf, int m, int pc) const {
        return *reinterpret_cast<const u32x4*>(buf + pc * PIECEB + (wo * W::MT + m) * BLKB + c_lane);
    }
    __device__ __forceinline__ u32x4 fragB(const char* buf, int n, int pc) const {
        return *reinterpret_cast<const u32x4*>(buf + OPERB + pc * PIECEB + (wi * W::NTL + n) * BLKB + c_lane);
    }
    __device__ __forceinline__ void flush_bias(float* dB) const {     // sum the four column groups of a quad first
        if (p_oper != 0 || t.i_off != 0) return;
        auto red = [&](float v, int f) {
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            if (p_cg == 0) atomicAdd(dB + 4 * p_fq + f, v);
        };
        red(bacc.x, 0); red(bacc.y, 1); red(bacc.z, 2); red(bacc.w, 3);
    }
};

// Tile granules: the operands are read the way the sweeps write them — wave pw (0..3 of its operand) stages feature tiles
// 4 pw .. 4 pw + 3, lane = (q, li) holding features 16 T + 4 q .. + 3 of column li.
// FX = true: the operands arrive as 24-bit tile-major stash arrays (dudf_internal.h "p24": [layer][feature tile][16-column group]
// [64 lanes][3 dwords]) of FIXED-POINT values relative to a per-layer, per-column power of two 2^E: value = (t - 3) 2^E with
// t = 0x40000000 | the 24 bits.  The lane's column is fixed for a stage, so ONE extra dword per lane and stage (`sc`) brings 2^E,
// and one FMA per value — t * g - 3 g with g = 2^E x the operand's layer scale — yields the number the fp16 split starts from.
// A 16-column stage of an operand is 16 contiguous 768-byte blocks, one per feature tile: a wave loads a block with ONE dwordx3
// instruction (six full lines).
// FX = false: the fp32 row layout — a wave-instruction takes 256-byte pieces of FOUR feature-quad rows (row 16 pw + 4 t + q,
// column li) instead of 64-byte pieces of sixteen — without the 24-bit decode ("row-major staging").
// A lane therefore has many features of ONE column — the transpose of what the MFMA wants (one feature, 8 columns) — so the
// LDS image is [column k][feature] (rows of 576 bytes: 256 fp16 + 64, four consecutive rows start 16 banks apart; the
// 8-byte unit index of a row XORed in its low three bits with (k >> 1) & 7: a 16-lane ds_write_b64 service group covers
// the 32 write banks once) and the fragments come out of it through ds_read_b64_tr_b16, gfx950's transposing LDS read: a
// 16-lane group reads 4 rows (columns k) x 16 features and every lane receives its feature's four k — two of them per
// fragment (tools/micro/tr_image.hip checks image, swizzle and fragment maps against a host GEMM).
template <bool FX>
struct TileStager : StagerBase {
    static constexpr int NPC = 2;                           // an fp16x3 stager: hi / lo
    static constexpr int ROWB = 576;                        // one column's 256 fp16 + 64 bytes
    static constexpr int PIECEB = 16 * ROWB;                // 9 KiB
    static constexpr int OPERB = NPC * PIECEB;              // 18 KiB
    static constexpr int BUFB = 2 * OPERB;                  // 36 KiB
    static constexpr int kSetLoads = FX ? 5 : 4;            // FX: + the column scale
    typedef unsigned u3_t __attribute__((ext_vector_type(3)));
    typedef typename std::conditional<FX, u3_t, f32x4>::type raw_t;      // FX: a granule is 3 dwords (four 24-bit values)
    struct RawSet { raw_t g0, g1, g2, g3; float sc; };      // granule j: tile 4 pw + j, column li; sc (FX): the column's 2^E
    // (FX: a layer of a 24-bit array is 3/4 of stash_layer floats; H == Hs, so the tile's row offsets are 0)
    __device__ static __forceinline__ int64_t layer_stride(const WgradArgs& a) { return FX ? a.stash_layer / 4 * 3 : a.stash_layer; }
    __device__ static __forceinline__ void drain(RawSet& r0, RawSet& r1, RawSet& r2) {      // everything in flight has landed
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(r0.g0), "+v"(r0.g1), "+v"(r0.g2), "+v"(r0.g3), "+v"(r1.g0), "+v"(r1.g1),
                     "+v"(r1.g2), "+v"(r1.g3), "+v"(r2.g0), "+v"(r2.g1), "+v"(r2.g2), "+v"(r2.g3));
        if constexpr (FX) asm volatile("" : "+v"(r0.sc), "+v"(r1.sc), "+v"(r2.sc));
    }

    int pw, p_q, p_li;
    unsigned t_voff0, t_vstep, p_li4;
    int t_w0, t_w1;                 // image write offsets of this lane: tiles with even / odd t
    int c_t0, c_t1;                 // ... and its two transposed reads of a fragment
    const float *F0, *F1;           // FX: the column scales of the wave's operands (layer j + 1 for q / zbar, layer j for A / s)
    f32x4 bacc[4] = {};             // bias gradient partial sums: one quad of features per tile
    __device__ __forceinline__ TileStager(const WgradArgs& a_, const WgTile& t_, char* ldsb_, int tid, int wave)
        : StagerBase(a_, t_, ldsb_, tid, wave) {
        const int lane = tid & 63, j = t.j;
        F0 = FX ? (p_oper ? a.fxA + (int64_t)j * a.np : a.fxQ + (int64_t)(j + 1) * a.np) : nullptr;
        F1 = FX ? (p_oper ? a.fxS + (int64_t)j * a.np : a.fxZ + (int64_t)(j + 1) * a.np) : nullptr;
        pw = wave & (NW_ / 2 - 1); p_q = lane >> 4; p_li = lane & 15;
        const int64_t ngrp = a.np >> 4;                                       // 16-column groups per row of tiles
        // FX: tile 4 pw (+ t) of the tile-major array; else row 16 pw + q (+ 4 t) of the fp32 row layout, column li
        t_voff0 = FX ? (unsigned)(lane * 12 + (int64_t)(4 * pw) * ngrp * 768)   // (the launcher keeps a layer below 2^32 bytes)
                     : (unsigned)((((int64_t)(16 * pw + p_q)) * a.np + p_li) * 16);
        t_vstep = FX ? (unsigned)(ngrp * 768) : (unsigned)(4 * a.np * 16);
        p_li4 = (unsigned)p_li * 4u;                                           // FX: this lane's column scale inside a stage's 16
        // row li, unit 16 pw + 4 t + q with its low three bits swizzled
        const int p_sw = (p_li >> 1) & 7;
        t_w0 = p_oper * OPERB + p_li * ROWB + 128 * pw + 8 * (p_q ^ p_sw);
        t_w1 = p_oper * OPERB + p_li * ROWB + 128 * pw + 8 * ((4 + p_q) ^ p_sw);
        // rows k = 8 (lane >> 5) + ((lane & 15) >> 2) and k + 4, unit 8 b + 4 ((lane >> 4) & 1) + (lane & 3) of block b, low
        // three bits swizzled with the row's (k >> 1) & 7
        // (FX: the same two numbers written through (q, li) — with the lane form hipcc folds the row index of that build
        //  differently and its three-buffer hot loop gains a v_add_u32; the fp32-row build is the other way round)
        const int c_k = FX ? 8 * (p_q >> 1) + (p_li >> 2) : 8 * (lane >> 5) + ((lane & 15) >> 2);
        const int c_u = FX ? 4 * (p_q & 1) + (p_li & 3) : 4 * ((lane >> 4) & 1) + (lane & 3);
        c_t0 = c_k * ROWB + 8 * (c_u ^ ((c_k >> 1) & 7));
        c_t1 = (c_k + 4) * ROWB + 8 * (c_u ^ (((c_k + 4) >> 1) & 7));
    }
    __device__ __forceinline__ const char* stage_src(int it) const {          // wave-uniform: this stage's 16 columns of the operand
        return reinterpret_cast<const char*>(operand(it)) + (int64_t)t.step_of(it) * (FX ? 768 : KB * 16);
    }
    __device__ __forceinline__ void load(int it, RawSet& r) const {
        const uint64_t sbase = wg_uniform64(stage_src(it));
        if constexpr (FX) {
            const uint64_t fbase = wg_uniform64((t.pair_of(it) ? F1 : F0) + (int64_t)t.step_of(it) * KB);
            asm volatile("global_load_dwordx3 %0, %5, %9\n\tglobal_load_dwordx3 %1, %6, %9\n\t"
                         "global_load_dwordx3 %2, %7, %9\n\tglobal_load_dwordx3 %3, %8, %9\n\t"
                         "global_load_dword %4, %10, %11"
                         : "=&v"(r.g0), "=&v"(r.g1), "=&v"(r.g2), "=&v"(r.g3), "=&v"(r.sc)
                         : "v"(t_voff0), "v"(t_voff0 + t_vstep), "v"(t_voff0 + 2 * t_vstep), "v"(t_voff0 + 3 * t_vstep), "s"(sbase),
                           "v"(p_li4), "s"(fbase) : "memory");
        } else {
            asm volatile("global_load_dwordx4 %0, %4, %8\n\tglobal_load_dwordx4 %1, %5, %8\n\t"
                         "global_load_dwordx4 %2, %6, %8\n\tglobal_load_dwordx4 %3, %7, %8"
                         : "=&v"(r.g0), "=&v"(r.g1), "=&v"(r.g2), "=&v"(r.g3)
                         : "v"(t_voff0), "v"(t_voff0 + t_vstep), "v"(t_voff0 + 2 * t_vstep), "v"(t_voff0 + 3 * t_vstep), "s"(sbase) : "memory");
        }
    }
    __device__ __forceinline__ void load_plain(int it, RawSet& r) const {     // (ordinary loads: see RowStager)
        const char* src = stage_src(it) + t_voff0;
        r.g0 = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(src));
        r.g1 = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(src + t_vstep));
        r.g2 = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(src + 2 * (size_t)t_vstep));
        r.g3 = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(src + 3 * (size_t)t_vstep));
        if constexpr (FX) r.sc = (t.pair_of(it) ? F1 : F0)[(int64_t)t.step_of(it) * KB + p_li];
    }
    template <int N>
    __device__ static __forceinline__ void wait(RawSet& r) {
        if constexpr (FX) asm volatile("s_waitcnt vmcnt(%5)" : "+v"(r.g0), "+v"(r.g1), "+v"(r.g2), "+v"(r.g3), "+v"(r.sc) : "n"(N));
        else asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r.g0), "+v"(r.g1), "+v"(r.g2), "+v"(r.g3) : "n"(N));
    }
    // tile tt of this lane's four (features 16 (4 pw + tt) + 4 q .. + 3 of column li): unpack, bias sums, fp16 hi / lo, two
    // 8-byte writes into row li of the image
    // (FX: `scl` = 2^E of this lane's column x the operand's layer scale, `m3` = -3 scl: v = (t - 3) scl is the value in the GEMM's
    //  scale, the bias sums run in that scale too and are divided by the layer scale at the end)
    __device__ __forceinline__ void split_tile(const raw_t& g, int tt, int bsel, const float bmask, const float scl, const float m3) {
        f32x4 v;
        f16x2 h0, h1;
        if constexpr (FX) {
            const u32x4 p = fx24_patterns(g[0], g[1], g[2]);
            v = f32x4{__builtin_fmaf(__uint_as_float(p[0]), scl, m3), __builtin_fmaf(__uint_as_float(p[1]), scl, m3),
                      __builtin_fmaf(__uint_as_float(p[2]), scl, m3), __builtin_fmaf(__uint_as_float(p[3]), scl, m3)};
            h0 = __builtin_convertvector(f32x2{v[0], v[1]}, f16x2); h1 = __builtin_convertvector(f32x2{v[2], v[3]}, f16x2);
        } else {
            v = g;
        }
        bacc[tt] += bmask * v;
        const f32x2 v0 = {v[0], v[1]}, v1 = {v[2], v[3]};
        char* dst = ldsb + bsel * BUFB + ((tt & 1) ? t_w1 : t_w0) + 64 * (tt >> 1);
        if constexpr (FX) {
            put_hi_lo<PIECEB>(dst, f16_hi_lo(v0, v1, h0, h1));
        } else {
            // hi = fp16(v 2^k) in ONE instruction per value (v_fma_mixlo_f16 / v_fma_mixhi_f16: fp32 sources, fp16 result into one
            // half of the destination; the product with a power of two is exact, so this is the rounding of multiply + convert)
            asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h0) : "v"(v0.x), "s"(scl));
            asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h0) : "v"(v0.y), "s"(scl));
            asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h1) : "v"(v1.x), "s"(scl));
            asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h1) : "v"(v1.y), "s"(scl));
            put_hi_lo<PIECEB>(dst, f16_hi_lo(v0, v1, h0, h1, scl));
        }
    }
    __device__ __forceinline__ void split_store(int it, const RawSet& r, int bsel) {
        const float bmask = bias_mask(it);
        const float scl0 = layer_scale(it);
        const float scl = FX ? r.sc * scl0 : scl0;          // FX: per lane — the column's 2^E times the layer scale (both powers of two)
        const float m3 = -3.0f * scl;
        split_tile(r.g0, 0, bsel, bmask, scl, m3); split_tile(r.g1, 1, bsel, bmask, scl, m3);
        split_tile(r.g2, 2, bsel, bmask, scl, m3); split_tile(r.g3, 3, bsel, bmask, scl, m3);
    }
    __device__ __forceinline__ u32x4 frag_tr(const char* base) const {
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + c_t0)));
        const u32x2 hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + c_t1)));
        return u32x4{lo.x, lo.y, hi.x, hi.y};
    }
    __device__ __forceinline__ u32x4 fragA(const char* buf, int m, int pc) const { return frag_tr(buf + pc * PIECEB + (wo * W::MT + m) * 64); }
    __device__ __forceinline__ u32x4 fragB(const char* buf, int n, int pc) const { return frag_tr(buf + (OPERB + pc * PIECEB + n * 64) + wi * (W::NTL * 64)); }
    __device__ __forceinline__ void flush_bias(float* dB) const {     // the 16 columns (lanes li) of features 16 (4 pw + tt) + 4 q + e
        if (p_oper != 0 || t.i_off != 0) return;
        const float bun = FX ? 1.0f / sc1 : 1.0f;           // FX: the sums ran in zbar's layer scale (a power of two)
        auto red = [&](float v, int f) {
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
            if (p_li == 0) atomicAdd(dB + f, v * bun);
        };
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int e = 0; e < 4; ++e) red(bacc[tt][e], 16 * (4 * pw + tt) + 4 * p_q + e);
    }
};

// The flags: per-buffer stage counters in LDS instead of a workgroup barrier per stage.  A wave starts stage `it` when all
// eight waves have written their part of image `it` (counter W) and have finished reading the buffer its own split is about
// to overwrite (counter R): waves may drift up to a stage apart, so the SIMD partner that the issue arbitration serves first
// (the older wave) no longer idles a third of every stage at the barrier while the younger one finishes.
// NB = 3: a wave must ask — a second poll per stage — whether every wave has finished READING image it - 1 before it splits
// image it + 2 into that buffer.  NB = 4: the buffer of image it + 2 is the one image it - 2 lived in, and the poll at the top
// of stage `it` (every wave has WRITTEN image it, which it does behind its reads of image it - 2: LDS executes a wave's
// operations in order) already says so: one poll and one flag less per stage.
// Per-wave progress words in LDS (no atomics, no address registers).  A wave publishes with ds_write_addtid_b32 from lane 0
// (address M0) and polls the whole block with one ds_read_addtid_b32 (lane i reads word i).  Inline asm: the poll is a
// loop, and a compiler-visible loop inside the hand-counted stage loop makes hipcc spill registers that still have loads
// in flight.
__device__ __forceinline__ void wg_publish(unsigned lds_addr, unsigned value) {
    unsigned keep, vt; uint64_t ex;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_mov_b64 %2, exec\n\ts_mov_b64 exec, 1\n\t"
                 "v_mov_b32 %1, %4\n\tds_write_addtid_b32 %1\n\ts_mov_b64 exec, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&v"(vt), "=&s"(ex) : "s"(lds_addr), "s"(value) : "memory");
}
// one block of 24 words at flag0: lanes 0-7 = images written by waves 0..7, 8-15 = stages whose fragment reads are finished,
// 16-23 = stages whose MFMAs are nearly all issued.  All three are plain stage counters.
__device__ __forceinline__ void wg_poll(unsigned flag0, unsigned need_w, unsigned need_r, unsigned need_h03, unsigned need_h47) {
    unsigned keep, vt, t0, t1;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n"
                 ".Ldudf_poll%=:\n\t"
                 "ds_read_addtid_b32 %1\n\ts_waitcnt lgkmcnt(0)\n\t"
                 "v_cmp_le_u32 vcc, %5, %1\n\ts_and_b32 %2, vcc_lo, 0xff\n\t"
                 "v_cmp_le_u32 vcc, %6, %1\n\ts_and_b32 %3, vcc_lo, 0xff00\n\ts_or_b32 %2, %2, %3\n\t"
                 "v_cmp_le_u32 vcc, %7, %1\n\ts_and_b32 %3, vcc_lo, 0xf0000\n\ts_or_b32 %2, %2, %3\n\t"
                 "v_cmp_le_u32 vcc, %8, %1\n\ts_and_b32 %3, vcc_lo, 0xf00000\n\ts_or_b32 %2, %2, %3\n\t"
                 "s_cmp_eq_u32 %2, 0xffffff\n\t"
                 "s_cbranch_scc1 .Ldudf_done%=\n\ts_sleep 1\n\ts_branch .Ldudf_poll%=\n"
                 ".Ldudf_done%=:\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep), "=&v"(vt), "=&s"(t0), "=&s"(t1)
                 : "s"(flag0), "s"(need_w), "s"(need_r), "s"(need_h03), "s"(need_h47) : "memory", "vcc", "scc");
}

// NB: image buffers in LDS, 3 or 4 (see the flags above); SP: 0 = bf16x6, 1 = fp16x3 MFMA groups
template <int H, int NB, int SP, class Stager>
__device__ __forceinline__ void wgrad_pipeline(const WgradArgs& a) {
    using W = WG<H>;
    static_assert(H == 256 && (NB == 3 || NB == 4), "256 x 256 output tiles, three or four images");
    static_assert(Stager::NPC == (SP ? 2 : 3), "the stager writes the pieces the MFMA groups read: TileStager is an fp16x3 stager");
    using RawSet = typename Stager::RawSet;
    constexpr int NPC = Stager::NPC;                        // pieces per operand
    constexpr int NW_ = W::WO * W::WI;
    constexpr int BUFB = Stager::BUFB;
    extern __shared__ __attribute__((aligned(16))) char ldsb[];     // [NB image buffers: X | Y, each NPC pieces], then the flags

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave / W::WI, wi = wave % W::WI;
    // Layers wider than the tile (512: 2 x 2 tiles): the four tiles of one (layer, column split) read the same X rows twice
    // and the same Y rows twice.  On a 1-D grid whose blocks are dealt round-robin over the 8 XCDs, blocks with equal id % 8
    // share an XCD and its L2: a group's tiles get ids xcd + 8 * (4 * (group / 8) + tile), so the second reader of every row
    // hits L2 instead of HBM (PMC r03_b: 15.2 GB fetched per launch at 8x512 / 125 000 points against 7.2 GB of operands).
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, nsplit = gridDim.y;
    if (a.remap_nsplit > 0) {
        const int id = blockIdx.x, slot = id >> 3, grp = (slot >> 2) * 8 + (id & 7);
        if (grp >= a.nj * a.remap_nsplit) return;               // the grid is padded to whole XCD rounds
        bz = slot & 3; bx = grp % a.nj; by = grp / a.nj; nsplit = a.remap_nsplit;
    }
    const WgTile t(a, H, bx, by, bz, nsplit, a.steps_total * (KT / KB), Stager::layer_stride(a));
    const int j = t.j, nit = t.nit;
    // (fp16x3 build only: the bf16x6 build sits at 256 registers and four more live scalars make it spill)
    const bool clk_on = SP != 0 && a.clk != nullptr && bx == 0 && by == 0 && bz == 0;
    const unsigned long long clk_t0 = clk_on ? __builtin_amdgcn_s_memtime() : 0ull, clk_r0 = clk_on ? __builtin_amdgcn_s_memrealtime() : 0ull;

    f32x16 acc[W::MT][W::NTL];
    wg_zero(acc);
    // fp16x3: this wave's operand scale for each pair (waves 0..3 stage X, 4..7 stage Y), and the common product scale 2^P of the layer
    Stager st(a, t, ldsb, tid, wave);
    float inv_p = 1.f;
    if constexpr (SP != 0) {
        const int oper = st.p_oper;
        const int eq = dudf_exp_above(a.amax[0 * a.L + j + 1]), eA = dudf_exp_above(a.amax[1 * a.L + j]);
        const int ez = dudf_exp_above(a.amax[2 * a.L + j + 1]);
        const int esh = dudf_exp_above(a.amax[3 * a.L + j]);             // h | hdot^k of the Hessian quads; plain columns: |h| <= 1 (+ an ulp)
        const int es = esh > 1 ? esh : 1;
        const int P1l = 30 - eq - eA, P2l = 30 - ez - es;
        const int P = (a.have_g && P1l < P2l) ? P1l : P2l;
        // the pair with the larger admissible product gives the surplus back through its X operand
        st.sc0 = oper ? dudf_pow2(15 - eA) : dudf_pow2(15 - eq - (P1l - P));
        st.sc1 = oper ? dudf_pow2(15 - es) : dudf_pow2(15 - ez - (P2l - P));
        if (!a.have_g) st.sc0 = st.sc1;
        inv_p = dudf_pow2(-P);
    }
    RawSet R0, R1, R2;                                                    // stage s travels in set s % 3, three stages ahead
    const unsigned flag0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(ldsb + NB * BUFB);

    if (tid < 128) reinterpret_cast<unsigned*>(ldsb + NB * BUFB)[tid] = 0;
    __syncthreads();
    if (nit > 0) {                                       // images 0 and 1 written, images 2, 3, 4 in flight (image k: set k % 3)
        st.load_plain(0, R0);
        if (nit > 1) st.load_plain(1, R1);
        if (nit > 2) st.load_plain(2, R2);
        st.split_store(0, R0, 0);
        wg_publish(flag0 + 4u * (unsigned)wave, 1u);                           // one image written
        if (nit > 3) st.load_plain(3, R0);
        if (nit > 1) {
            st.split_store(1, R1, 1);
            wg_publish(flag0 + 4u * (unsigned)wave, 2u);                       // two
        }
        if (nit > 4) st.load_plain(4, R1);
    }
    __syncthreads();
    // one stage: 48 MFMAs, then the registers of the stage two further on -> pieces (that set is then refilled with the stage
    // three further on, so three stages = 96 KiB per CU stay in flight: with one, the kernel measured latency-bound at 2 TB/s)
    auto stage = [&](int it, RawSet& r, auto hot, auto bidx) {
        constexpr int BI = decltype(bidx)::value;             // it % 3 (the loops advance by three stages)
        const char* buf = ldsb + (NB == 4 ? (it & 3) : BI) * BUFB;
        constexpr bool HOT = decltype(hot)::value;
        {
            // every wave has written its part of image `it` (generation g + 1 of W[BI]) and has finished reading image
            // it - 1, whose buffer this wave's split of image it + 2 is going to overwrite (R[(BI + 2) % 3])
            // (the second condition is checked in front of the split, behind this stage's MFMAs: the SIMD partner runs half
            //  a stage behind, and waiting for ITS reads here would stall this wave at the top of every stage)
            // + the SIMD partners alternate on the matrix pipe: waves 4-7 start the MFMAs of stage `it` when waves 0-3 have
            //   issued most of theirs, waves 0-3 start stage `it` when waves 4-7 have issued most of stage it - 1 (the flag is
            //   raised one MFMA group before the end, so that the hand-over latency is covered)
            const unsigned uit = (unsigned)it;
            const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(wave >= NW_ / 2));
            wg_poll(flag0, uit + 1u, 0u, hi ? uit + 1u : 0u, hi ? 0u : uit);
        }
        u32x4 af[W::MT][NPC], bn[NPC];
#pragma unroll
        for (int m = 0; m < W::MT; ++m)
#pragma unroll
            for (int pc = 0; pc < NPC; ++pc) af[m][pc] = st.fragA(buf, m, pc);
#pragma unroll
        for (int pc = 0; pc < NPC; ++pc) bn[pc] = st.fragB(buf, 0, pc);
#pragma unroll
        for (int n = 0; n < W::NTL; ++n) {
            u32x4 bc[NPC];
#pragma unroll
            for (int pc = 0; pc < NPC; ++pc) bc[pc] = bn[pc];
            if (n + 1 < W::NTL) {
#pragma unroll
                for (int pc = 0; pc < NPC; ++pc) bn[pc] = st.fragB(buf, n + 1, pc);
                __builtin_amdgcn_sched_barrier(0x76);        // LDS reads and MFMAs keep their order: fragments one block ahead
            }
#pragma unroll
            for (int m = 0; m < W::MT; ++m) {
                f32x16 c = acc[m][n];
                if constexpr (SP != 0) {                          // smallest terms first: lo*hi, hi*lo, hi*hi
                    auto H8 = [](u32x4 v) { return __builtin_bit_cast(f16x8, v); };
                    c = mfma_f16(H8(af[m][1]), H8(bc[0]), c);
                    c = mfma_f16(H8(af[m][0]), H8(bc[1]), c);
                    c = mfma_f16(H8(af[m][0]), H8(bc[0]), c);
                } else {
                    auto B8 = [](u32x4 v) { return __builtin_bit_cast(bf16x8, v); };
                    const bf16x8 bh = B8(bc[0]), bmid = B8(bc[1]), bl = B8(bc[NPC - 1]);
                    c = mfma_bf16(B8(af[m][1]), bmid, c);             // smallest terms first
                    c = mfma_bf16(B8(af[m][NPC - 1]), bh, c);
                    c = mfma_bf16(B8(af[m][0]), bl, c);
                    c = mfma_bf16(B8(af[m][1]), bh, c);
                    c = mfma_bf16(B8(af[m][0]), bmid, c);
                    c = mfma_bf16(B8(af[m][0]), bh, c);
                }
                acc[m][n] = c;
            }
            if (n == W::NTL - kHandOver) {
                __builtin_amdgcn_sched_barrier(0);
                wg_publish(flag0 + 64u + 4u * (unsigned)wave, (unsigned)it + 1u);                  // nearly done with the matrix pipe
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // behind this stage's last fragment reads (LDS executes a wave's operations in order): image `it` read; then
        // the split of image it + 2 into the buffer image it - 1 (NB = 4: it - 2) lived in, and its flag
        __builtin_amdgcn_sched_barrier(0);
        const int BW = NB == 4 ? ((it + 2) & 3) : (BI + 2) % 3;
        if constexpr (NB == 3) {
            wg_publish(flag0 + 32u + 4u * (unsigned)wave, (unsigned)it + 1u);                    // fragment reads of stage `it` done
            if (HOT || it + 2 < nit) wg_poll(flag0, 0u, (unsigned)it, 0u, 0u);                   // image it - 1 read by everybody: its buffer is free
        }
        if constexpr (HOT) {
            Stager::template wait<2 * Stager::kSetLoads>(r);                                     // the two younger sets stay in flight
            st.split_store(it + 2, r, BW);
            st.load(it + 5, r);
            wg_publish(flag0 + 4u * (unsigned)wave, (unsigned)it + 3u);                          // images 0 .. it + 2 written
        } else if (it + 2 < nit) {
            st.split_store(it + 2, r, BW);
            if (it + 5 < nit) st.load_plain(it + 5, r);
            wg_publish(flag0 + 4u * (unsigned)wave, (unsigned)it + 3u);
        }
    };
    int it = 0;
    const int nhot = nit >= 8 ? ((nit - 5) / 3) * 3 : 0;
    // hipcc does not know the sets are in flight: enter (and leave) the hand-counted loop with everything landed, so that
    // the register copies it places on the loop's edges are harmless; inside, the sets stay put (tests/isa_contract.py
    // replays the loop body twice and fails on any instruction that touches a register with a load in flight)
    Stager::drain(R0, R1, R2);
    using B0 = std::integral_constant<int, 0>; using B1 = std::integral_constant<int, 1>; using B2 = std::integral_constant<int, 2>;
    // register set of a stage: that of the image it splits, it + 2 (set (it + 2) % 3)
    for (; it < nhot; it += 3) {
        stage(it, R2, std::true_type{}, B0{});
        stage(it + 1, R0, std::true_type{}, B1{});
        stage(it + 2, R1, std::true_type{}, B2{});
    }
    Stager::drain(R0, R1, R2);
    for (; it < nit; it += 3) {
        stage(it, R2, std::false_type{}, B0{});
        if (it + 1 < nit) stage(it + 1, R0, std::false_type{}, B1{});
        if (it + 2 < nit) stage(it + 2, R1, std::false_type{}, B2{});
    }

    float* dW = t.dW(a);
    float* dB = t.dB(a);
    if (nit > 0) {
        wg_add_tile<H>(a, dW, wo, wi, acc, inv_p);           // (bf16x6: inv_p is the literal 1)
        st.flush_bias(dB);
    }
    if (clk_on && tid == 0) {
        a.clk[0] = __builtin_amdgcn_s_memtime() - clk_t0;
        a.clk[1] = __builtin_amdgcn_s_memrealtime() - clk_r0;
    }
}
// built without packed fp32 instructions (dudf_internal.h, DUDF_NO_PK): the split slices of one wave then execute beside its
// SIMD partner's MFMAs (-5 % on this kernel).  The pipeline and the stagers' members are forced-inline functions: lambdas
// defined inside a function that carries the target attribute do not inherit it and would not be inlined.
// VAR in the kernels' names (profiles, DESIGN.md and the tests know them by it): 9 = three image buffers, 25 = four.
template <int VAR> constexpr int wg_buffers() { static_assert(VAR == 9 || VAR == 25, "VAR 9: three image buffers, 25: four"); return VAR == 25 ? 4 : 3; }
template <int H, int VAR>
__global__ __launch_bounds__(64 * WG<H>::WO * WG<H>::WI) DUDF_NO_PK void wgrad_hidden_bf16p_kernel(WgradArgs a) { wgrad_pipeline<H, wg_buffers<VAR>(), 0, RowStager<0>>(a); }
template <int H, int VAR>
__global__ __launch_bounds__(64 * WG<H>::WO * WG<H>::WI) DUDF_NO_PK void wgrad_hidden_f16p_kernel(WgradArgs a) { wgrad_pipeline<H, wg_buffers<VAR>(), 1, RowStager<1>>(a); }
// ... the fp32 rows staged 4 rows x 256 bytes per wave-instruction
template <int H, int VAR>
__global__ __launch_bounds__(64 * WG<H>::WO * WG<H>::WI) DUDF_NO_PK void wgrad_hidden_f16tr_kernel(WgradArgs a) { wgrad_pipeline<H, wg_buffers<VAR>(), 1, TileStager<false>>(a); }
// ... reading 24-bit tile-major operands (dudf_internal.h "p24")
template <int H, int VAR>
__global__ __launch_bounds__(64 * WG<H>::WO * WG<H>::WI) DUDF_NO_PK void wgrad_hidden_f16p24_kernel(WgradArgs a) { wgrad_pipeline<H, wg_buffers<VAR>(), 1, TileStager<true>>(a); }

// ---- first and last layer: thin reductions over columns (bandwidth-bound, VALU) -------------------------
//   dW_1[o][d] | db_1[o] = sum_c  q_1[o][c] * gbar[c][d]  +  zbar_1[o][c] * x4[c][d]      (d = 3 is the bias: x4[c][3])
//   dW_out[f]            = sum_c  A_L[f][c] * x4[c][3]   +  ybar[c] * s_L[f][c]
//   db_out               = sum_c  ybar[c]
#ifndef DUDF_WGSMALL_P24_PTS
#define DUDF_WGSMALL_P24_PTS 4096
#endif
struct WgradSmallArgs {
    const float *Q, *A, *Z, *S;
    const float *x4, *gbar, *ybar;      // x4 [np][4]; gbar [np][4]; ybar [np]
    float* dtheta;
    int64_t np, ncols, stash_layer, off_wo, off_bo;
    int H, L, have_g;
    int pts_per_block;
    float rho;                          // w0 / ww: d(loss)/d(W_1, b_1) = rho d(loss)/d(rho W_1, rho b_1)
    const float *fxS, *fxQ, *fxA, *fxZ; // 24-bit fixed-point arrays: [L][np] column scales (dudf_internal.h)
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid.x = column ranges, grid.y = feature-quad groups; block = 256 threads = 4 waves; each wave loops over
// feature quads, lanes run over 64 consecutive columns (16-byte granules -> 1 KiB coalesced per load).
__device__ __forceinline__ void wgrad_small_body(const WgradSmallArgs& a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int FQ = a.H / 4;
    const int64_t p0 = (int64_t)blockIdx.x * a.pts_per_block;
    const int64_t p1 = (p0 + a.pts_per_block < a.ncols) ? p0 + a.pts_per_block : a.ncols;
    const float* Q0 = a.Q;                                          // layer index 0
    const float* Z0 = a.Z;
    const float* AL = a.A + (int64_t)(a.L - 1) * a.stash_layer;
    const float* SL = a.S + (int64_t)(a.L - 1) * a.stash_layer;
    const int fq_per = (FQ + gridDim.y - 1) / gridDim.y;
    const int fq_lo = blockIdx.y * fq_per, fq_hi = (fq_lo + fq_per < FQ) ? fq_lo + fq_per : FQ;
    for (int fq = fq_lo + wave; fq < fq_hi; fq += 4) {
        float w1[4][4], wo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { wo[c] = 0.f; w1[c][0] = w1[c][1] = w1[c][2] = w1[c][3] = 0.f; }
#pragma unroll 4
        for (int64_t p = p0 + lane; p < p1; p += 64) {
            const int64_t off = ((int64_t)fq * a.np + p) * 4;
            // the stash is a stream (last reader of these rows); x4 / gbar / ybar are re-read per feature quad: cached
            const f32x4 z = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Z0 + off));
            const f32x4 sl = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(SL + off));
            const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x4 + p * 4);
            const float yb = a.ybar[p];
            f32x4 qv = {0, 0, 0, 0}, al = {0, 0, 0, 0}, gb = {0, 0, 0, 0};
            if (a.have_g) {
                qv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Q0 + off));
                al = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(AL + off));
                gb = *reinterpret_cast<const f32x4*>(a.gbar + p * 4);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int d = 0; d < 4; ++d) w1[c][d] += qv[c] * gb[d] + z[c] * xv[d];
                wo[c] += al[c] * xv[3] + yb * sl[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int f = 4 * fq + c;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const float v = wave_sum(w1[c][d]);
                if (lane == 0) atomicAdd(d < 3 ? a.dtheta + f * 3 + d : a.dtheta + 3 * a.H + f, a.rho * v);
            }
            const float vo = wave_sum(wo[c]);
            if (lane == 0) atomicAdd(a.dtheta + a.off_wo + f, vo);
        }
    }
    if (wave == 0 && blockIdx.y == 0) {                               // db_out = sum ybar
        float s = 0.f;
        for (int64_t p = p0 + lane; p < p1; p += 64) s += a.ybar[p];
        s = wave_sum(s);
        if (lane == 0) atomicAdd(a.dtheta + a.off_bo, s);
    }
}
__global__ __launch_bounds__(256) DUDF_NO_PK void wgrad_small_kernel(WgradSmallArgs a) { wgrad_small_body(a); }

// The same reduction over the 24-bit tile-major fixed-point arrays (dudf_internal.h "p24" bit 0): grid.x = column ranges, grid.y =
// feature tiles; a wave walks 16-column groups, lane = (q, li) as in the sweeps: ONE dwordx3 per array and group (768 contiguous
// bytes per wave) + the column's scale 2^E; value = (t - 3) 2^E (dudf_sweep_common.h fx24_pack).
__device__ __forceinline__ f32x4 small_unpack24(const unsigned* g, const float sc) {
    typedef unsigned u3_t __attribute__((ext_vector_type(3)));
    const u3_t d = __builtin_nontemporal_load(reinterpret_cast<const u3_t*>(g));
    // (the decode of fx24_patterns, dudf_internal.h, written out: through the shared helper this kernel — 223 registers and a
    //  64-byte spill slot — comes out with another instruction order and measured 0.5 us slower)
    const unsigned d0 = d.x, d1 = d.y, d2 = d.z;
    const unsigned m = 0x00ffffffu, two = 0x40000000u;
    const unsigned y = __builtin_amdgcn_perm(d1, d0, 0x0c0c0703u);
    const unsigned t3 = __builtin_amdgcn_perm(d2, y, 0x0c070100u) | two;
    const float m3 = -3.0f * sc;
    return f32x4{__builtin_fmaf(__uint_as_float((d0 & m) | two), sc, m3), __builtin_fmaf(__uint_as_float((d1 & m) | two), sc, m3),
                 __builtin_fmaf(__uint_as_float((d2 & m) | two), sc, m3), __builtin_fmaf(__uint_as_float(t3), sc, m3)};
}
__global__ __launch_bounds__(256) DUDF_NO_PK void wgrad_small_p24_kernel(WgradSmallArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, li = lane & 15, T = blockIdx.y;
    const int64_t ng = a.np >> 4;
    const int64_t g0 = (int64_t)blockIdx.x * (a.pts_per_block >> 4);
    const int64_t gend = (a.ncols + 15) >> 4;
    const int64_t g1 = g0 + (a.pts_per_block >> 4) < gend ? g0 + (a.pts_per_block >> 4) : gend;
    const int64_t lbytes = a.stash_layer * 3;                            // bytes per layer of a 24-bit array
    auto tile = [&](const float* arr, int layer) { return reinterpret_cast<const char*>(arr) + (int64_t)layer * lbytes + (int64_t)T * ng * 768 + lane * 12; };
    const char* Q0 = tile(a.Q, 0); const char* Z0 = tile(a.Z, 0);
    const char* AL = tile(a.A, a.L - 1); const char* SL = tile(a.S, a.L - 1);
    float w1[4][4], wo[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { wo[c] = 0.f; w1[c][0] = w1[c][1] = w1[c][2] = w1[c][3] = 0.f; }
    float sy = 0.f;
    const int nwave = (int)(blockDim.x >> 6);                           // 4; ONE in the deterministic mode (one adder per output)
#pragma unroll 4
    for (int64_t g = g0 + wave; g < g1; g += nwave) {
        const int64_t p = g * 16 + li;
        const f32x4 z = small_unpack24(reinterpret_cast<const unsigned*>(Z0 + g * 768), a.fxZ[p]);
        const f32x4 sl = small_unpack24(reinterpret_cast<const unsigned*>(SL + g * 768), a.fxS[(int64_t)(a.L - 1) * a.np + p]);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x4 + p * 4);
        const float yb = a.ybar[p];
        f32x4 qv = {0, 0, 0, 0}, al = {0, 0, 0, 0}, gb = {0, 0, 0, 0};
        if (a.have_g) {
            qv = small_unpack24(reinterpret_cast<const unsigned*>(Q0 + g * 768), a.fxQ[p]);
            al = small_unpack24(reinterpret_cast<const unsigned*>(AL + g * 768), a.fxA[(int64_t)(a.L - 1) * a.np + p]);
            gb = *reinterpret_cast<const f32x4*>(a.gbar + p * 4);
        }
        sy += yb;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int d = 0; d < 4; ++d) w1[c][d] += qv[c] * gb[d] + z[c] * xv[d];
            wo[c] += al[c] * xv[3] + yb * sl[c];
        }
    }
    auto sum16 = [](float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); return v; };
    // the block's waves add up in LDS first: one atomic per output and BLOCK instead of one per wave (400 blocks x 4 waves x 80
    // atomics onto 1280 addresses were a fifth of this kernel's time)
    __shared__ float red[4][4][21];                                      // [wave][lane quarter][20 sums + sum of ybar]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const float v = sum16(w1[c][d]);
            if (li == 0) red[wave][q][c * 4 + d] = v;
        }
        const float vo = sum16(wo[c]);
        if (li == 0) red[wave][q][16 + c] = vo;
    }
    {
        const float v = sum16(sy);
        if (li == 0) red[wave][q][20] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 81; t += blockDim.x) {                 // (one wave per block in the deterministic mode)
        if (t < 80) {                                                    // (q, c, d | output row): the waves' partial sums -> one atomic
            const int qq = t / 20, k = t % 20;
            float v = 0.f;
            for (int w = 0; w < nwave; ++w) v += red[w][qq][k];
            if (k < 16) {
                const int c = k >> 2, d = k & 3, f = 16 * T + 4 * qq + c;
                atomicAdd(d < 3 ? a.dtheta + f * 3 + d : a.dtheta + 3 * a.H + f, a.rho * v);
            } else {
                atomicAdd(a.dtheta + a.off_wo + 16 * T + 4 * qq + (k - 16), v);
            }
        } else if (T == 0) {                                             // db_out = sum ybar (every quarter holds the same sum)
            float v = 0.f;
            for (int w = 0; w < nwave; ++w) v += red[w][0][20];
            atomicAdd(a.dtheta + a.off_bo, v);
        }
    }
}

static_assert(KTP == 33 && NRING == 4 && KB == 16, "dudf_choose_wgrad: LDS sizes");
template <int H>
int launch_hidden(const SweepChoice& c, const WgradArgs& a, hipStream_t st) {
    using W = WG<H>;
    const int tz = a.Hs / H, ntz = tz * tz;              // output tiles of a layer wider than the 256 x 256 tile
    // one resident workgroup per CU, a single round.  dudf_set_wgrad_max_workgroups (default 256) caps the grid: with more
    // than one rank the engine sets 240, so that an RCCL kernel queued behind the previous layer group finds free CUs
    // beside this GEMM (its workgroups fill the register file of the CUs they run on)
    int nsplit = dudf_wgrad_max_workgroups() / (a.nj * ntz);
    if (nsplit > a.steps_total) nsplit = a.steps_total;
    if (nsplit < 1 || dudf_deterministic()) nsplit = 1;      // deterministic: one workgroup per weight tile, one add per element
    const dim3 grid(a.nj, nsplit, ntz), block(64 * W::WO * W::WI);
    if (c.family == DUDF_FAM_WG_F32) return dudf_launch_kernel<&wgrad_hidden_kernel<H>>(grid, block, c.lds, c.lds_max, st, a);
    if (c.family == DUDF_FAM_WG_BF16) return dudf_launch_kernel<&wgrad_hidden_bf16_kernel<H>>(grid, block, c.lds, c.lds_max, st, a);
    if constexpr (H == 256) {                                // the cooperative-split kernels
        if (c.family == DUDF_FAM_WG_F16P24 && c.fl == 25) return dudf_launch_kernel<&wgrad_hidden_f16p24_kernel<H, 25>>(grid, block, c.lds, c.lds_max, st, a);
        if (c.family == DUDF_FAM_WG_F16P24) return dudf_launch_kernel<&wgrad_hidden_f16p24_kernel<H, 9>>(grid, block, c.lds, c.lds_max, st, a);
        if (c.family == DUDF_FAM_WG_F16TR) return dudf_launch_kernel<&wgrad_hidden_f16tr_kernel<H, 9>>(grid, block, c.lds, c.lds_max, st, a);
        if (c.family == DUDF_FAM_WG_BF16P) return dudf_launch_kernel<&wgrad_hidden_bf16p_kernel<H, 9>>(grid, block, c.lds, c.lds_max, st, a);
        if (c.family == DUDF_FAM_WG_F16P && c.remap) {       // 2 x 2 tiles: a group's tiles on one XCD
            WgradArgs b = a;
            b.remap_nsplit = nsplit;
            return dudf_launch_kernel<&wgrad_hidden_f16p_kernel<H, 9>>(dim3(((a.nj * nsplit + 7) / 8) * 32), block, c.lds, c.lds_max, st, b);
        }
        if (c.family == DUDF_FAM_WG_F16P) return dudf_launch_kernel<&wgrad_hidden_f16p_kernel<H, 9>>(grid, block, c.lds, c.lds_max, st, a);
    }
    return DUDF_E_UNSUPPORTED;
}

}  // namespace

// dW / db of the layers [layer_begin, layer_end) in theta order: 0 = first layer (3 -> H), 1 .. L-1 = hidden matrices,
// L = output layer.  The two thin layers share one kernel (one pass over the columns): it runs when either is asked for.
int dudf_launch_wgrad(const DudfLayout& lo, float* ws, float* dtheta, int have_g, hipStream_t st, int layer_begin,
                      int layer_end) {
    if (layer_begin < 0) layer_begin = 0;
    if (layer_end > lo.L + 1) layer_end = lo.L + 1;
    WgradArgs a;
    a.Q = ws + lo.ws_Q; a.A = ws + lo.ws_A; a.Z = ws + lo.ws_Z; a.S = ws + lo.ws_S; a.ncol_h = lo.ncol_h;
    a.dtheta = dtheta; a.np = lo.np; a.stash_layer = lo.stash_layer;
    a.off_hid = lo.off_hid; a.hid_stride = lo.hid_stride; a.steps_total = (int)(lo.ncols / KT); a.L = lo.L;
    a.have_g = have_g; a.Hs = lo.H;
    a.amax = reinterpret_cast<const unsigned*>(ws + lo.ws_amax);
    a.clk = dudf_prof_clk(PROF_WGRAD_HIDDEN);
    a.remap_nsplit = 0;
    a.fxS = ws + lo.ws_fx[0]; a.fxQ = ws + lo.ws_fx[1]; a.fxA = ws + lo.ws_fx[2]; a.fxZ = ws + lo.ws_fx[3];
    const int hb = layer_begin < 1 ? 1 : layer_begin, he = layer_end > lo.L ? lo.L : layer_end;   // hidden matrices asked for
    a.j0 = hb - 1; a.nj = he > hb ? he - hb : 0;
    int rc = 0;
    if (a.nj > 0) {
        DudfProfScope prof(PROF_WGRAD_HIDDEN, st);
        const SweepChoice c = dudf_choose_wgrad(WgradRequest{lo.H, lo.L, lo.p24 & 1, lo.np}, dudf_options());
        if (c.status) return c.status;
        dudf_note_products(PROF_WGRAD_HIDDEN, c.products);
        switch (c.H) {
            case 32: rc = launch_hidden<32>(c, a, st); break;
            case 64: rc = launch_hidden<64>(c, a, st); break;
            case 128: rc = launch_hidden<128>(c, a, st); break;
            default: rc = launch_hidden<256>(c, a, st); break;
        }
    }
    if (rc) return rc;
    if (!(layer_begin <= 0 || layer_end >= lo.L + 1)) return 0;     // neither thin layer in range
    WgradSmallArgs s;
    s.Q = a.Q; s.A = a.A; s.Z = a.Z; s.S = a.S; s.x4 = ws + lo.ws_x4; s.gbar = ws + lo.ws_gbar; s.ybar = ws + lo.ws_ybar;
    s.dtheta = dtheta; s.np = lo.np; s.ncols = lo.ncols; s.stash_layer = lo.stash_layer;
    s.off_wo = lo.off_wo; s.off_bo = lo.off_bo; s.H = lo.H; s.L = lo.L; s.have_g = have_g; s.rho = lo.rho;
    s.fxS = a.fxS; s.fxQ = a.fxQ; s.fxA = a.fxA; s.fxZ = a.fxZ;
    s.pts_per_block = dudf_deterministic() ? (int)lo.ncols : 4096;     // with 16 feature-quad groups 4096 columns per block measured best (0.096 ms; 1024 x 4 groups: 0.156)
    const int grid = (int)((lo.ncols + s.pts_per_block - 1) / s.pts_per_block);
    DudfProfScope prof(PROF_WGRAD_SMALL, st);
    const int fqn = lo.H / 4;                                              // feature quads; a block's 4 waves take one each per round:
    const int gy = fqn >= 64 ? 16 : (fqn >= 4 ? fqn / 4 : 1);              // up to 16 groups -> more loads in flight per CU
    if (lo.p24 & 1) {                               // 24-bit tile-major arrays: one block row per feature tile, whole groups per block
        if (!dudf_deterministic()) {
            // (more blocks than the fp32 kernel: the decode + scale loads make a wave's chain longer.)  Large batches: 4096 columns
            // per block; the reference's batch (29 970 columns: 8 x 16 blocks, half the CUs idle, 74 us against 86 us at 100 000)
            // gets at least ~30 column blocks, in multiples of 256 columns
            s.pts_per_block = DUDF_WGSMALL_P24_PTS;
            const int64_t want = (lo.ncols / 30 + 255) / 256 * 256;
            if (want < s.pts_per_block) s.pts_per_block = want < 512 ? 512 : (int)want;
        }
        s.pts_per_block = (s.pts_per_block + 15) / 16 * 16;
        hipLaunchKernelGGL(wgrad_small_p24_kernel, dim3((unsigned)((lo.ncols + s.pts_per_block - 1) / s.pts_per_block), lo.H / 16),
                           dim3(dudf_deterministic() ? 64 : 256), 0, st, s);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(wgrad_small_kernel, dim3(grid, gy), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}
