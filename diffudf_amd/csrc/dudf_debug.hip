// Diagnostic doors to the per-point code of a training step: the 3x3 eigensolver on matrices of the caller's choosing, and the loss
// stage (loss_fwd / loss_bwd / the loss_s2 statistics, dudf_loss.hip) on planted (y, df/dx, Hessian) without a sweep in front of it or
// an adjoint sweep behind it.  A unit of its own: the production kernels and launchers are called, not changed.  See include/dudf_hip.h.
#include "dudf_context.h"
#include "dudf_eigh3.h"

namespace {

constexpr int kGridCap = 2048;

__global__ __launch_bounds__(256) void debug_eigh3_kernel(const double* __restrict__ H, int64_t k, double* __restrict__ out_lam,
                                                          double* __restrict__ out_V) {
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < k; m += (int64_t)gridDim.x * blockDim.x) {
        double Hm[3][3], lam[3], V[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Hm[i][j] = H[m * 9 + i * 3 + j];
        eigh3(Hm, lam, V);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            out_lam[m * 3 + i] = lam[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) out_V[m * 9 + i * 3 + j] = V[i][j];
        }
    }
}

// which point a column belongs to, and as what: channel 0 = the point itself, 1..3 = Hessian column k = channel - 1 of a quad,
// -1 = padding (quad padding behind n_h, plain padding behind n)
struct ColumnRole { int64_t p; int ch; };
__device__ __forceinline__ ColumnRole role_of(int64_t c, int64_t n, int64_t n_h, int64_t ncol_h) {
    if (c < ncol_h) {
        const int64_t p = c >> 2;
        return p < n_h ? ColumnRole{p, (int)(c & 3)} : ColumnRole{-1, -1};
    }
    const int64_t p = n_h + (c - ncol_h);
    return p < n ? ColumnRole{p, 0} : ColumnRole{-1, -1};
}

// per POINT -> per column: the inverse of copy_out_kernel.  Hessian: g[(4p+1+k)*4 + i] = h[p][i][k].  What no kernel of the loss stage
// may read — padded columns, and the y of a quad's tangent channels (a sweep leaves d y / d x_k there) — is NaN.
__global__ __launch_bounds__(256) void debug_scatter_kernel(const float* __restrict__ y, const float* __restrict__ g,
                                                            const float* __restrict__ h, float* __restrict__ wy, float* __restrict__ wg,
                                                            int64_t n, int64_t n_h, int64_t ncol_h, int64_t ncols) {
    const float nan = __builtin_nanf("");
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * blockDim.x) {
        const ColumnRole r = role_of(c, n, n_h, ncol_h);
        float yv = nan;
        f32x4 gv = {nan, nan, nan, nan};
        if (r.ch == 0) {
            yv = y[r.p];
            gv = f32x4{g[r.p * 3], g[r.p * 3 + 1], g[r.p * 3 + 2], 0.f};
        } else if (r.ch > 0) {
            const int k = r.ch - 1;
            gv = f32x4{h[r.p * 9 + k], h[r.p * 9 + 3 + k], h[r.p * 9 + 6 + k], 0.f};
        }
        wy[c] = yv;
        *reinterpret_cast<f32x4*>(wg + c * 4) = gv;
    }
}

// per column -> per POINT: out_hbar[p][i][k] from column 4p+1+k.  Every float the loss stage owes a zero — all five of a padded
// column, ybar of a quad's tangent channels, the fourth gbar float of any column — is looked at bit by bit; a column with one that
// is not +0 counts once.
__global__ __launch_bounds__(256) void debug_gather_kernel(const float* __restrict__ wyb, const float* __restrict__ wgb,
                                                           float* __restrict__ ybar, float* __restrict__ gbar, float* __restrict__ hbar,
                                                           int* __restrict__ pad_nonzero, int64_t n, int64_t n_h, int64_t ncol_h,
                                                           int64_t ncols) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * blockDim.x) {
        const ColumnRole r = role_of(c, n, n_h, ncol_h);
        const float yv = wyb[c];
        const f32x4 gv = *reinterpret_cast<const f32x4*>(wgb + c * 4);
        unsigned owed = __float_as_uint(gv[3]);
        if (r.ch == 0) {
            ybar[r.p] = yv;
            gbar[r.p * 3] = gv[0]; gbar[r.p * 3 + 1] = gv[1]; gbar[r.p * 3 + 2] = gv[2];
        } else if (r.ch > 0) {
            const int k = r.ch - 1;
            hbar[r.p * 9 + k] = gv[0]; hbar[r.p * 9 + 3 + k] = gv[1]; hbar[r.p * 9 + 6 + k] = gv[2];
            owed |= __float_as_uint(yv);
        } else {
            owed |= __float_as_uint(yv) | __float_as_uint(gv[0]) | __float_as_uint(gv[1]) | __float_as_uint(gv[2]);
        }
        if (owed != 0u) atomicAdd(pad_nonzero, 1);
    }
}

// check_loss_mode's rules (dudf_api.hip) for a call that runs the forward and the backward of one mode: the three modes, loss_s2 with
// somewhere to put its statistics, Hessian-path points only under loss_s1 with a Hessian weight
int check_stage_mode(int mode, int64_t n_hess, const double* weights, const double* stats) {
    if (mode != DUDF_LOSS_S1 && mode != DUDF_LOSS_SIREN && mode != DUDF_LOSS_S2) return DUDF_E_BADMODE;
    if (mode == DUDF_LOSS_S2 && !stats) return DUDF_E_BADMODE;
    if (n_hess != 0 && !(mode == DUDF_LOSS_S1 && weights[2] != 0.0)) return DUDF_E_BADMODE;
    return 0;
}

}  // namespace

extern "C" {

int dudf_debug_eigh3(const double* H, int64_t k, double* out_lam, double* out_V, void* stream) {
    if (k < 0) return DUDF_E_BADCFG;
    if (k == 0) return 0;
    if (!H || !out_lam || !out_V) return DUDF_E_BADCFG;
    return dudf_launch(debug_eigh3_kernel, dim3(dudf_grid_for(k, 256, kGridCap)), dim3(256), reinterpret_cast<hipStream_t>(stream), H, k,
                       out_lam, out_V);
}

int dudf_debug_loss_stage(const dudf_net_cfg* cfg, int mode, int64_t n, int64_t n_hess, const float* y, const float* g, const float* h,
                          const float* normals, const float* sdf, int64_t n_global, const double* weights, double alpha,
                          const float* cot, const double* stats_in, float* out_terms, double* out_stats, float* out_ybar,
                          float* out_gbar, float* out_hbar, int* out_pad_nonzero, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (!weights) return DUDF_E_BADCFG;
    DUDF_TRY(check_stage_mode(mode, n_hess, weights, out_stats));
    DudfCtx c;
    DUDF_TRY(dudf_open_ctx(cfg, n, n_hess, workspace, workspace_bytes, stream, &c));
    if (n_global < 1 && n > 0) return DUDF_E_BADCFG;
    if (n == 0) return 0;
    if (!y || !g || !normals || !sdf || !cot || !out_terms || !out_ybar || !out_gbar || !out_pad_nonzero) return DUDF_E_BADCFG;
    if (n_hess > 0 && (!h || !out_hbar)) return DUDF_E_BADCFG;
    const DudfLayout& lo = c.lo;
    float* ws = c.ws;
    const dim3 grid(dudf_grid_for(lo.ncols, 256, kGridCap)), block(256);
    DUDF_TRY(dudf_launch(debug_scatter_kernel, grid, block, c.st, y, g, h, ws + lo.ws_y, ws + lo.ws_g, lo.n, lo.n_h, lo.ncol_h, lo.ncols));
    DUDF_TRY(hipMemsetAsync(ws + lo.ws_acc, 0, (size_t)2 * DUDF_NACC * sizeof(float), c.st));   // as the forward's fallback path does
    DUDF_TRY(hipMemsetAsync(ws + lo.ws_ybar, 0xff, (size_t)lo.np * sizeof(float), c.st));         // a NaN in every float
    DUDF_TRY(hipMemsetAsync(ws + lo.ws_gbar, 0xff, (size_t)4 * lo.np * sizeof(float), c.st));
    DUDF_TRY(hipMemsetAsync(out_terms, 0, 4 * sizeof(float), c.st));
    DUDF_TRY(hipMemsetAsync(out_pad_nonzero, 0, sizeof(int), c.st));
    const double* stats = nullptr;
    if (mode == DUDF_LOSS_S2) {
        DUDF_TRY(dudf_launch_s2_stats(lo, sdf, ws, out_stats, c.st));
        DUDF_TRY(dudf_launch_s2_terms(out_stats, weights, out_terms, c.st));
        stats = stats_in ? stats_in : out_stats;
    } else {
        DUDF_TRY(dudf_launch_loss_fwd(lo, mode, normals, sdf, n_global, weights, alpha, ws, out_terms, c.st));
    }
    DUDF_TRY(dudf_launch_loss_bwd(lo, mode, normals, sdf, n_global, weights, alpha, cot, stats, ws, c.st));
    return dudf_launch(debug_gather_kernel, grid, block, c.st, ws + lo.ws_ybar, ws + lo.ws_gbar, out_ybar, out_gbar, out_hbar,
                       out_pad_nonzero, lo.n, lo.n_h, lo.ncol_h, lo.ncols);
}

}  // extern "C"
