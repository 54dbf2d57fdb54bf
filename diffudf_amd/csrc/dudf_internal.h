// Internal layout shared by the kernels and the C-ABI glue (not installed; see include/dudf_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/dudf_hip.h"
#include "dudf_variants.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned cvt_pk(f32x2 v) {              // one v_cvt_pk_bf16_f32: lo = bf16(v.x), hi = bf16(v.y)
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ f32x2 unpack(unsigned p) {              // the two bf16 back as exact floats
    return f32x2{__builtin_bit_cast(float, p << 16), __builtin_bit_cast(float, p & 0xffff0000u)};
}
// The three dwords of a 24-bit fixed-point granule (dudf_sweep_common.h c24_pack / fx24_pack: values 0-2 in the low three
// bytes of a dword each, value 3 spread over the three top bytes) -> the four bit patterns t = 0x40000000 | 24 bits, floats in [2, 4]
__device__ __forceinline__ u32x4 fx24_patterns(unsigned d0, unsigned d1, unsigned d2) {
    const unsigned m = 0x00ffffffu, two = 0x40000000u;                                     // (the pattern of 2.0f: an inline constant)
    const unsigned t0 = (d0 & m) | two, t1 = (d1 & m) | two, t2 = (d2 & m) | two;          // v_and_or_b32
    const unsigned y = __builtin_amdgcn_perm(d1, d0, 0x0c0c0703u);                        // [d0.b3, d1.b3, 0, 0]
    const unsigned t3 = __builtin_amdgcn_perm(d2, y, 0x0c070100u) | two;                   // [.., .., d2.b3, 0] | 0x40 on top
    return u32x4{t0, t1, t2, t3};
}

#define DUDF_TILE_PTS 64           // columns per workgroup pass of the f32 sweep kernel (4 waves x 16)
#define DUDF_COL_PAD 128           // column ranges are padded to this: the bf16 sweep kernel's pass (8 waves x 16)
#define DUDF_NACC 16               // doubles in the reduction scratch

// Everything is in units of floats unless it says bytes.
//
// theta (caller's flat parameters, reference state_dict order):
//   [W_1 (H,3)] [b_1 (H)] { [W_l (H,H)] [b_l (H)] } l=2..L  [W_out (1,H)] [b_out (1)]
//
// COLUMNS.  The sweeps and the weight-gradient GEMM work on "columns" of the activation matrices.
//   * a point on the plain path (value + df/dx) is ONE column;
//   * a point on the Hessian path is FOUR adjacent columns (a quad): channel 0 = the value path, channels 1..3 =
//     the tangents d/dx_k of every forward and reverse quantity (forward-over-reverse).  The
//     matmuls are linear, so tangents are just more columns of the same MFMAs; only the elementwise tails couple
//     the four lanes of a quad (DPP quad broadcasts / sums).
//   column ranges: [0, ncol_h) Hessian quads of the first n_h points, [ncol_h, ncol_h + ncol_n) plain columns of
//   the remaining n - n_h points; both padded to whole 128-column tiles with zero columns.
//
// workspace:
//   w1b    [H][4]      = rho [W_1 | b_1]    A-operand of the first layer (bias folded in as k=3); rho = w0 / ww (1 unless ww != w0)
//   b1s    [L][H]      = rho b_1 | b_2 | .. | b_L: the hidden layers' biases, contiguous per layer (the forward tails index it by layer)
//   w1t16  [16][H]     rows 0..2 = rho W_1^T, rest 0: A-operand of the last reverse step (df/dx)
//   wt     [L-1][H][H] W_l^T for l=2..L     A-operand of the reverse sweeps (f32 kernel)
//   wimg   bf16x3 images of W_l, then of W_l^T, in A-fragment order (dudf_sweep16.h)
//   wimg16 fp16 hi/lo images of 2^k_l W_l, then of 2^k_l W_l^T (same order, two pieces; "fp16x3" split)
//   wsc    [2][L-1]: 2^-k_l (what the accumulators of matrix l are multiplied with), then 2^k_l
//   ebound [L][np]: max over the features of |e_l| per column (the adjoint forward sweep leaves it for the fp16x3 adjoint
//          reverse sweep, which scales each column of zbar_l = w0 c_l hbar_l - e_l by a power of two before it knows it)
//   amax   [4][L] uint: bit patterns of max |q_l|, |A_l|, |zbar_l|, |h_l| (Hessian quads) over all columns of the step (fp16x3 weight-gradient GEMM)
//   per column: x4 [np][4] = layer-1 B operand (x,1 | e_k,0), y [np], g [np][4] (a_0 rows), ybar [np], gbar [np][4]
//   stash arrays, each [L][H/4][np][4]:  element (layer li, feature f, column p) lives at
//       ((li*(H/4) + f/4)*np + p)*4 + f%4
//   i.e. "feature-quad major, column minor": the 16x16x4 MFMA accumulator of a wave (feature rows
//   4q..4q+3 of a tile in its 4 registers, column = lane&15) is one aligned 16-byte store per lane,
//   and the weight-gradient GEMM reads whole 16-byte [column][4 features] granules.
//     S  h_l   | hdot_l^k      (forward outputs: Y operand of wgrad)       C  cos(w0 z_l)
//     ZS s_l   | zdot_l^k      (Hessian columns only)                      Q  q_l | qdot_l^k   (X operand of wgrad)
//     R  r_l = w0^2 s_l a_l (plain)  |  a_l | adot_l^k (Hessian)          E  e_l (see dudf_sweep.hip)
//     A  A_l   | Adot_l^k      (Y operand of wgrad)                        Z  zbar_l | zdotbar_l^k (X operand)
//   acc: DUDF_NACC doubles of reduction scratch (loss sums, s2 statistics)
//
// "p24" stash (round 4; DudfLayout::p24, training workspaces of 256-wide networks whose sweeps and weight-gradient GEMM run
// their fp16x3 kernels; option stash = 0 keeps everything fp32): arrays that only the BACKWARD reads hold 24 bits per value, four
// values in 12 bytes.  R, E (bit 1): fp32 values rounded to 24 bits (sign, 8 exponent, 15 mantissa bits: relative error <= 2^-17).
// C (bit 2; read by the reverse sweep, whose df/dx has no precision to spare, cannot take a 2^-17 relative error, but |cos| <= 1
// needs no exponent): 24-bit FIXED POINT on a 2^-22 grid (absolute error <= 2^-23, the size of the sin/cos polynomials' own
// error; dudf_sweep_common.h c24_pack).  S, Q, A, Z (bit 0, round 5; the weight-gradient GEMM's operands — a 2^-17 relative error
// on them moved the 12-step trajectory by 4e-4): the same fixed point, relative to a per-layer, per-COLUMN power of two 2^E that
// the sweep leaves in the side arrays ws_fx (fx24_pack: absolute error <= 2^(E-23)).  ZS stays fp32.  A 12-byte granule per
// lane makes 192-byte row segments, every second cache line shared by two waves: measured, partial-line writes give back
// 15 of the 25 % (tools/micro/hbm_p24.hip, profiles/r04_hbm_p24.txt).  So these arrays are TILE-MAJOR instead:
//     [layer][feature tile T = f/16][column group g = p/16][lane = 16*((f%16)/4) + p%16][3 dwords]
// i.e. the 64 lanes of a wave write their accumulator tile as 768 contiguous bytes (six full lines):
//     byte offset of granule (layer, f, p) = (((layer*(H/16) + f/16)*(np/16) + p/16)*64 + 16*((f%16)/4) + p%16)*12
// dwords of a granule (values v0..v3 = features 4q..4q+3, u_i = bits(v_i) + 0x80):
//     d0 = u0>>8 | u1.byte1<<24,  d1 = u1>>16 | (u2>>8)<<16,  d2 = u2.byte3 | (u3>>8)<<8
// C: u_i = the low 24 bits of bits(c_i + 3.0f) = (c_i + 1) 2^22;  d_i = u_i | u3.byte_i << 24  (i = 0, 1, 2).  In the Hessian-quad columns C keeps one granule per quad: `p` above is then the quad's index p >> 2
// (groups [0, ncol_h/64), below the plain columns' groups, which start at ncol_h/16).
struct DudfLayout {
    int H, L;
    float rho;               // w0 / ww (dudf_net_cfg): the first layer is packed times rho, `w0` below is the ONE frequency the kernels run (ww)
    int p24;                 // which arrays are 24-bit tile-major (see above): bit 0 = S, Q, A, Z (the weight-gradient GEMM's operands), bit 1 = R, E, bit 2 = C (fixed point)
    float w0;
    int64_t n, n_h;          // points, and how many of them (the first n_h) take the Hessian path
    int64_t ncol_h, ncol_n;  // padded column counts of the two ranges
    int64_t ncols;           // ncol_h + ncol_n: columns the kernels process
    int64_t np;              // row stride of the per-column arrays, in columns (>= ncols)
    // theta
    int64_t off_w1, off_b1, off_hid, hid_stride, off_wo, off_bo, n_theta;
    // workspace
    int64_t ws_w1b, ws_b1s, ws_w1t16, ws_wt, ws_wimg, ws_wimg16, ws_wsc, ws_amax, ws_ebound, ws_zbound, ws_x4, ws_y, ws_g, ws_ybar, ws_gbar;
    int64_t ws_S, ws_C, ws_ZS, ws_Q, ws_R, ws_E, ws_A, ws_Z, ws_acc;
    int64_t ws_fx[4];        // p24 bit 0: column scales [L][np] of the fixed-point arrays S, Q, A, Z (in the order of the sweeps that write them)
    int64_t stash_layer;     // H*np: floats per layer in a stash array (p24 arrays: 3/4 of that, H*np*3 BYTES)
    size_t total_bytes;
};

// the current run-time options (dudf_set_option in the C ABI; dudf_runtime.hip holds them, dudf_variants.h lists them)
DudfOptions dudf_options();
inline bool dudf_deterministic() { return dudf_options().deterministic != 0; }
inline bool dudf_split_fp16() { return dudf_options().split != 0; }
inline int dudf_wgrad_max_workgroups() { return dudf_options().wgrad_max_workgroups; }

// carves arrays out of a buffer of floats: every array starts on a 64-float (256-byte) granule
struct DudfCarver { int64_t o; int64_t take(int64_t cnt) { const int64_t r = o; o += (cnt + 63) / 64 * 64; return r; } };

// workgroups of `block` threads for n items, at least 1 and at most `cap` (the kernels stride over the rest)
inline int dudf_grid_for(int64_t n, int block, int cap) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// bytes rounded up to a whole 256-byte granule; 0 stays 0
inline size_t dudf_round256(size_t b) { return (b + 255) / 256 * 256; }

static inline int dudf_make_layout(const dudf_net_cfg* cfg, int64_t n, int64_t n_h, DudfLayout* lo, int query_only = 0) {
    if (!cfg || cfg->n_in != 3 || cfg->n_hidden_layers < 1) return DUDF_E_BADCFG;
    const int H = cfg->hidden, L = cfg->n_hidden_layers;
    if (!(H == 32 || H == 64 || H == 128 || H == 256 || H == 512)) return DUDF_E_BADCFG;
    if (n < 0 || n_h < 0 || n_h > n) return DUDF_E_BADCFG;
    if (!(cfg->w0 > 0.f) || cfg->ww < 0.f) return DUDF_E_BADCFG;
    const float ww = cfg->ww > 0.f ? cfg->ww : cfg->w0;
    lo->H = H; lo->L = L; lo->w0 = ww; lo->rho = cfg->w0 / ww;
    lo->n = n; lo->n_h = n_h;
    lo->p24 = query_only ? 0 : dudf_stash_p24_enabled(H, L, dudf_options());   // option stash, and every kernel of the step must be the build that reads / writes it
    auto pad = [](int64_t c) { return (c + DUDF_COL_PAD - 1) / DUDF_COL_PAD * DUDF_COL_PAD; };
    lo->ncol_h = pad(4 * n_h);
    lo->ncol_n = pad(n - n_h);
    lo->np = lo->ncol_h + lo->ncol_n;
    if (lo->np == 0) { lo->ncol_n = DUDF_COL_PAD; lo->np = DUDF_COL_PAD; }
    lo->ncols = lo->np;
    // np is the STRIDE (in columns) between the feature-quad rows of every per-column array; ncols the columns processed.
    // np * 16 bytes a large power of two would put all rows of a stash array on the same HBM channels (measured: 131 072
    // columns ran 1.9x slower per point than 98 304): skew the rows by one 256-byte granule.  (Skewing EVERY size — the row
    // stride is always a multiple of 2 KiB — was measured in round 3 and changes nothing at 100 000 points.)
    if (lo->np % 2048 == 0) lo->np += 32;
    if (lo->np * 1024 >= (1ll << 32)) lo->p24 = 0;            // 32-bit lane byte offsets inside a layer of a stash array (the weight-gradient GEMM's staging loads)
    lo->off_w1 = 0; lo->off_b1 = 3 * (int64_t)H;
    lo->off_hid = 4 * (int64_t)H; lo->hid_stride = (int64_t)H * H + H;
    lo->off_wo = lo->off_hid + (L - 1) * lo->hid_stride; lo->off_bo = lo->off_wo + H;
    lo->n_theta = lo->off_bo + 1;
    // every array starts on a 256-byte boundary of the workspace (whose base the caller aligns to 256 B): a lane quarter's
    // 256-byte segment of a stash row is then exactly two 128-byte lines.  (Round 3 first put two small arrays of 64 + 128 bytes
    // in front of the stash: every segment straddled three lines, and FETCH_SIZE / WRITE_SIZE of all four sweeps read 9-12 %
    // above the algorithmic bytes until this was noticed — profiles/r03_a, r03_b against r02_c.)
    DudfCarver cv = {0};
    lo->ws_w1b = cv.take(4 * (int64_t)H);
    lo->ws_b1s = cv.take((int64_t)L * H);                             // rho b_1 | b_2 .. b_L (the forward tails' biases, one row per layer)
    lo->ws_w1t16 = cv.take(16 * (int64_t)H);
    lo->ws_wt = cv.take((int64_t)(L - 1) * H * H);
    lo->ws_wimg = cv.take((int64_t)(L - 1) * H * H * 3);      // bf16x3 images of W_l and W_l^T: 2 x 6 bytes per weight
    lo->ws_wimg16 = cv.take((int64_t)(L - 1) * H * H * 2);    // fp16 hi/lo images of W_l and W_l^T: 2 x 4 bytes per weight
    lo->ws_wsc = cv.take(2 * (int64_t)(L > 1 ? L - 1 : 1));
    lo->ws_amax = cv.take(4 * (int64_t)L);
    lo->ws_ebound = query_only ? lo->ws_amax : cv.take((int64_t)L * lo->np);   // [L][np]: max_f |e_l[f][column]| (fp16x3 adjoint reverse sweep)
    // [L][np]: max_f |zdot_l[f][column]| of the tangent columns of the Hessian quads (left by the fp16x3 forward sweep of the
    // quads for the column scales of the sweeps behind it); every workspace with Hessian-path points has it (training and queries)
    lo->ws_zbound = (n_h == 0) ? lo->ws_amax : cv.take((int64_t)L * lo->ncol_h);
    lo->ws_x4 = cv.take(4 * lo->np);
    lo->ws_y = cv.take(lo->np); lo->ws_g = cv.take(4 * lo->np);
    lo->ws_ybar = cv.take(lo->np); lo->ws_gbar = cv.take(4 * lo->np);
    lo->stash_layer = (int64_t)H * lo->np;
    const int64_t stash = (int64_t)L * lo->stash_layer;
    const int64_t stash_b = (lo->p24 & 1) ? stash / 4 * 3 : stash;   // S, Q, A, Z: 12 instead of 16 bytes per granule
    const int64_t stash_r = (lo->p24 & 2) ? stash / 4 * 3 : stash;   // R, E
    const int64_t stash_c = (lo->p24 & 4) ? stash / 4 * 3 : stash;   // C (fixed point)
    lo->ws_S = cv.take(stash_b); lo->ws_C = cv.take(stash_c);
    lo->ws_ZS = n_h > 0 ? cv.take(stash) : lo->ws_S;
    if (query_only) {        // value / df/dx / Hessian queries only ever touch S, C, ZS: 16-24 KB per column instead of 56-64
        lo->ws_Q = lo->ws_R = lo->ws_E = lo->ws_A = lo->ws_Z = lo->ws_S;
    } else {
        lo->ws_Q = cv.take(stash_b); lo->ws_R = cv.take(stash_r); lo->ws_E = cv.take(stash_r); lo->ws_A = cv.take(stash_b);
        lo->ws_Z = cv.take(stash_b);
    }
    for (int i = 0; i < 4; ++i) lo->ws_fx[i] = (lo->p24 & 1) ? cv.take((int64_t)L * lo->np) : lo->ws_amax;
    lo->ws_acc = cv.take(2 * DUDF_NACC);
    lo->total_bytes = (size_t)cv.o * sizeof(float);
    return 0;
}

// Kernels whose vector-ALU work should run BESIDE the SIMD partner's MFMAs are built without the packed fp32 instructions
// (v_pk_fma_f32, v_pk_add_f32 ...): those occupy the matrix pipe's slot (tools/micro/coissue.hip — 48 of them + 24 MFMAs
// take the sum of their times; the unpacked forms the maximum + 25 %).  Device pass only (the host pass has no such feature).
#if defined(__HIP_DEVICE_COMPILE__)
#define DUDF_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define DUDF_NO_PK
#endif

// ---- launchers implemented in the .hip translation units -------------------------------------
struct SweepArgs {
    const float* theta; const float* w1b; const float* b1s; const float* w1t16; const float* wt;   // b1s: [L][H] biases as packed (row 0 = rho b_1)
    const char* wimg_f; const char* wimg_t;   // bf16x3 weight images (forward / transposed), dudf_sweep16.h
    const char* wimg16_f; const char* wimg16_t;   // fp16 hi/lo weight images, scaled by 2^k_l per matrix
    const float* wsc;         // [2][L-1]: 2^-k_l | 2^k_l
    unsigned* amax;           // [4][L]: running maxima of |q_l|, |A_l|, |zbar_l|, |h_l| of the quads (bit patterns), or nullptr
    float* ebound;            // [L][np]: per layer and column, max over features of |e_l| (written by SWEEP_ADJ_FWD), or nullptr
    float* zbound;            // [L][ncol_h]: per layer and quad column, max over features of |zdot_l| (written by SWEEP_FWD_H, fp16x3), or nullptr
    int64_t nch;              // ncol_h: row stride of zbound
    unsigned long long* clk;  // profiling: [2] shader-clock / 100 MHz reference-clock ticks of workgroup 0's lifetime, or nullptr
    int split;                // bit s: sweep s (SWEEP_FWD .. SWEEP_ADJ_REV) of the plain columns runs the fp16x3 kernel (dudf_split_mask)
    const float* x4;          // [np][4]: layer-1 B operand per column
    float* y; float* g;       // [np], [np][4]
    const float* ybar; const float* gbar;
    float *S, *C, *ZS, *Q, *R, *E, *A, *Z;
    int64_t np, stash_layer;
    int tile0, ntiles;             // column range of this launch, in 64-column tiles
    int hess;                      // 1: the range holds Hessian quads
    int64_t off_hid, hid_stride, off_wo, off_bo;
    int L; float w0;
    int store_s, store_c, train;   // what the sweep has to leave behind
    int have_e;                    // reverse adjoint sweep: e_l was produced by SWEEP_ADJ_FWD
    int p24;                       // which stash arrays are 24-bit tile-major (DudfLayout::p24: bit 0 = S, Q, A, Z, bit 1 = R, E, bit 2 = C)
    float* fxs;                    // p24 bit 0: [L][np] — per layer and column, the power of two 2^E that turns the fixed-point values of the array
                                   // THIS sweep stores (S / Q / A / Z by sweep) back into numbers; written by the sweep, read by the weight-gradient kernels
};

// set-attribute-once + launch of one kernel instantiation.  The "once" is per process and per instantiation (the static below):
// hipFuncSetAttribute on every launch would be paid on the launch path.
template <auto Kernel, class... Args>
int dudf_launch_kernel(dim3 grid, dim3 block, size_t lds, size_t lds_max, hipStream_t st, const Args&... args) {
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return (int)hipGetLastError();
}

// the launchers take the kernel from a SweepChoice (dudf_variants.h: dudf_choose_sweep / dudf_choose_pair / dudf_choose_wgrad)
int dudf_launch_sweep(const SweepChoice& c, const SweepArgs& a, hipStream_t st);          // the f32-input MFMA family
int dudf_launch_sweep_bf16(const SweepChoice& c, const SweepArgs& a, hipStream_t st);     // the 16-bit-core families (H = 128, 256, 512)
int dudf_launch_sweep_wide(const SweepChoice& c, const SweepArgs& a, hipStream_t st);     // ... of which H = 512 (called by dudf_launch_sweep_bf16)
int dudf_launch_sweep_pair(const SweepChoice& c, const SweepArgs& aq, const SweepArgs& ap, hipStream_t st);   // quads + plain columns in one grid
int dudf_launch_pack_bf16(const DudfLayout& lo, const float* theta, float* ws, hipStream_t st);

int dudf_launch_pack(const DudfLayout& lo, const float* theta, float* ws, hipStream_t st);
int dudf_launch_wgrad(const DudfLayout& lo, float* ws, float* dtheta, int have_g, hipStream_t st, int layer_begin = 0,
                      int layer_end = 1 << 30);
int dudf_launch_make_x4(const DudfLayout& lo, const float* x, float* ws, hipStream_t st);
int dudf_launch_field_features(const DudfLayout& lo, const float* ws, int inverse_mode, double alpha, float* out_df,
                               float* out_vec, int* out_flag_count, float* out_lam, float* out_V, hipStream_t st);
int dudf_launch_loss_fwd(const DudfLayout& lo, int mode, const float* normals, const float* sdf, int64_t n_global,
                         const double* w, double alpha, float* ws, float* out_terms, hipStream_t st);
// zero_f / zero_fn: a buffer the kernel zeroes on its way (d(theta) in front of the weight-gradient atomics), or nullptr
int dudf_launch_loss_bwd(const DudfLayout& lo, int mode, const float* normals, const float* sdf, int64_t n_global,
                         const double* w, double alpha, const float* cot, const double* stats, float* ws,
                         hipStream_t st, float* zero_f = nullptr, int64_t zero_fn = 0);
// ONE launch in front of a training forward: A-operand forms of theta (thin layers, fp16 hi/lo images + their scales;
// bf16x3 images and W^T only when a kernel that reads them will run), x4 from the points, and zeros for the loss sums and
// the running maxima.  need: bit 0 = bf16x3 images, bit 1 = W_l^T (f32-input reverse sweeps)
int dudf_launch_prep(const DudfLayout& lo, const float* theta, const float* x, float* ws, int need, hipStream_t st);
int dudf_launch_s2_stats(const DudfLayout& lo, const float* sdf, float* ws, double* stats, hipStream_t st);
int dudf_launch_s2_terms(const double* stats, const double* w, float* out_terms, hipStream_t st);
void dudf_adam_factors(double lr, double b1, double b2, int64_t step, float* step_size, float* bc2_sqrt);
int dudf_launch_adam_sched(float* theta, const float* g, float* m, float* v, int64_t n, double b1, double b2, double eps,
                           const float* sched, int64_t n_rows, const int64_t* row, double gscale, hipStream_t st);
int dudf_launch_adam(float* theta, const float* g, float* m, float* v, int64_t n, double lr, double b1, double b2,
                     double eps, int64_t step, double gscale, hipStream_t st);
int dudf_launch_read_stash(const DudfLayout& lo, const float* src, int layer, int channel, float* out, hipStream_t st, int per_quad = 0, int p24 = 0,
                           const float* fx = nullptr);   // p24: 1 = 24-bit float, 2 = fixed point (C), 3 = fixed point x the column scales `fx` [L][np]
int dudf_launch_copy_in(const DudfLayout& lo, const float* ybar, const float* gbar, float* ws, hipStream_t st);
int dudf_launch_copy_out(const DudfLayout& lo, const float* ws, float* out_f, float* out_g, float* out_h,
                         hipStream_t st);
// x4 from double positions (sphere tracing, point projection; dudf_query.hip)
int dudf_launch_rays_x4(const DudfLayout& lo, const double* t0, float* ws, hipStream_t st);
// dudf_pointcloud.hip: ordered compaction / append behind a device row counter (scratch: 2 * dudf_pc_tiles(n) ints).  rows (or
// nullptr): rows[i] = the source row of the i-th row this call adds; dudf_render_gather gathers its hits and their image rows through it
int64_t dudf_pc_tiles(int64_t n);
int dudf_launch_pc_append(const unsigned char* flags, int64_t n, const double* src_a, const double* src_b, const float* src_f,
                          double* dst_a, double* dst_b, float* out_f, int* rows, int64_t capacity, int64_t quota, int64_t* counter,
                          int* scratch, hipStream_t st);

// products per algorithmic multiply of the kernel a launcher is about to start in profile slot `slot`: 1 = f32-input MFMA,
// 3 = fp16 hi/lo split, 6 = three-piece bf16 split (bench.py labels and prices its roofline from THIS, not from a table)
void dudf_note_products(int slot, int products);

// ---- optional per-kernel HIP-event timing (dudf_profile_* in the C ABI) -----------------------------------
enum { PROF_PACK = 0, PROF_SWEEP_FWD, PROF_SWEEP_REV, PROF_SWEEP_ADJ_FWD, PROF_SWEEP_ADJ_REV, PROF_WGRAD_HIDDEN,
       PROF_WGRAD_SMALL, PROF_LOSS_FWD, PROF_LOSS_BWD, PROF_ADAM, PROF_OTHER, PROF_NSLOTS };
// device slot [2] where the kernel of `slot` leaves (s_memtime, s_memrealtime) deltas of its first workgroup while the
// profiler is on (nullptr otherwise): the clock the chip actually held under that kernel (dudf_profile_clocks)
unsigned long long* dudf_prof_clk(int slot);
void dudf_prof_begin(int slot, hipStream_t st);
void dudf_prof_end(int slot, hipStream_t st);
struct DudfProfScope {
    int slot; hipStream_t st;
    DudfProfScope(int s, hipStream_t t) : slot(s), st(t) { dudf_prof_begin(slot, st); }
    ~DudfProfScope() { dudf_prof_end(slot, st); }
};
