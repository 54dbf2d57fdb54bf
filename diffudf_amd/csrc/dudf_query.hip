// Queries behind the C ABI with their kernels: value / df/dx / Hessian / eigen-frame / curvature of points, fields on a regular
// grid, sphere tracing (marching and descent).  The sweeps themselves are sequenced through dudf_context.h.
#include "dudf_context.h"
#include "dudf_eigh3.h"

namespace {

// out_f (n), out_g (n,3), out_h (n,3,3) [Hessian points first n_h only meaningful], any may be null
__global__ __launch_bounds__(256) void copy_out_kernel(const float* __restrict__ y, const float* __restrict__ g,
                                                       float* __restrict__ of, float* __restrict__ og,
                                                       float* __restrict__ oh, int64_t n, int64_t n_h, int64_t ncol_h) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = p < n_h ? 4 * p : ncol_h + (p - n_h);
        if (of) of[p] = y[c];
        if (og) { og[p * 3] = g[c * 4]; og[p * 3 + 1] = g[c * 4 + 1]; og[p * 3 + 2] = g[c * 4 + 2]; }
        if (oh && p < n_h) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < 3; ++i) oh[p * 9 + i * 3 + k] = g[(c + 1 + k) * 4 + i];
        }
    }
}

// x4 of a regular N^3 grid on [-1,1]^3, linear index start+c, first axis slowest — the sample order of reference
// src/render_mc.py:36-49 (`extract_fields`); coordinates are index-derived, nothing is read from HBM.
__global__ __launch_bounds__(256) void make_x4_grid_kernel(float* __restrict__ x4, int64_t n, int64_t np, int64_t N,
                                                           int64_t start) {
    const float voxel = 2.0f / (float)(N - 1);
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < np; c += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = {0, 0, 0, 0};
        if (c < n) {
            const int64_t i = start + c;
            const int64_t i2 = i % N, i1 = (i / N) % N, i0 = (i / N / N) % N;
            v = f32x4{(float)i0 * voxel - 1.0f, (float)i1 * voxel - 1.0f, (float)i2 * voxel - 1.0f, 1.f};
        }
        *reinterpret_cast<f32x4*>(x4 + c * 4) = v;
    }
}

// Per-point features the renderers derive from (f, df/dx, Hessian):
//   out_df  = inverse(gt_mode, |f|, alpha)                    reference src/inverses.py:3-21 via src/render_mc.py:71
//   out_vec = -normalize(df/dx) (eps 1e-12)                    reference src/render_mc.py:74-75
//   flags   : points whose NORMALISED gradient has norm < 0.04 (only a vanishing gradient does, :86-93): the caller
//             re-queries those with the Hessian path for the eigenvector fallback
//   out_lam / out_V (Hessian points): eigenvalues ascending and eigenvectors (columns) of the Hessian's lower triangle,
//             reference src/render_st.py:57-62 `compute_normals_and_cd` (normal = V[:,2])
__global__ __launch_bounds__(256) void field_features_kernel(const float* __restrict__ y, const float* __restrict__ g,
                                                             int64_t n, int64_t n_h, int64_t ncol_h, int inverse_mode,
                                                             float alpha, double sqrt_alpha, float* __restrict__ out_df,
                                                             float* __restrict__ out_vec, int* __restrict__ flag_count,
                                                             float* __restrict__ out_lam, float* __restrict__ out_V) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = p < n_h ? 4 * p : ncol_h + (p - n_h);
        if (out_df) {
            const float f = fabsf(y[c]);
            float d;
            if (inverse_mode == 0) d = (f < 1.0f / alpha) ? sqrtf(f / alpha) : f;          // 'tanh'
            else if (inverse_mode == 1) d = (f > 0.f) ? f : 0.01f;                        // 'siren' (min_step 0.01)
            else d = (float)((double)((f > 0.f) ? sqrtf(f) : 0.01f) / sqrt_alpha);        // 'squared': the division in double
            out_df[p] = d;
        }
        if (out_vec) {
            const float gx = g[c * 4], gy = g[c * 4 + 1], gz = g[c * 4 + 2];
            const float nrm = sqrtf(gx * gx + gy * gy + gz * gz);
            const float inv = -1.0f / fmaxf(nrm, 1e-12f);
            const float vx = gx * inv, vy = gy * inv, vz = gz * inv;
            out_vec[p * 3] = vx; out_vec[p * 3 + 1] = vy; out_vec[p * 3 + 2] = vz;
            if (flag_count && sqrtf(vx * vx + vy * vy + vz * vz) < 0.04f) atomicAdd(flag_count, 1);
        }
        if ((out_lam || out_V) && p < n_h) {
            double Hm[3][3], lam[3], V[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Hm[0][k] = g[(c + 1 + k) * 4]; Hm[1][k] = g[(c + 1 + k) * 4 + 1]; Hm[2][k] = g[(c + 1 + k) * 4 + 2];
            }
            eigh3(Hm, lam, V);
            if (out_lam) { out_lam[p * 3] = (float)lam[0]; out_lam[p * 3 + 1] = (float)lam[1]; out_lam[p * 3 + 2] = (float)lam[2]; }
            if (out_V)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) out_V[p * 9 + i * 3 + j] = (float)V[i][j];
        }
    }
}

// ---- third-order jets for the curvature query (reference src/render_st.py:42-55) ------------------------------------
// One 16-column tile per point: column 0 = (x, 1), columns 1..3 = the eigen-frame A = v_0, B = v_1, C = v_2 = n of the
// Hessian as directions, the rest zero; SWEEP_FWD_J (dudf_sweep.hip) turns them into the Taylor coefficients y_m of
// f(x + sA + rB + tC) for the monomials listed there.  Mixed third derivatives in the frame:
//   T(A,A,C) = 2 y_sst, T(B,B,C) = 2 y_rrt, T(A,B,C) = y_srt, T(A,C,C) = 2 y_stt, T(B,C,C) = 2 y_rtt
// and the shape operator  J_ik = dn_i/dx_k = sum_{j<2} (v_j)_i T(v_j, n, e_k) / (lam_2 - lam_j)  (first-order perturbation
// of the top eigenvector of the Hessian — what autograd through torch.linalg.eigh returns), e_k expanded in the frame.
// mean = tr J / 2 = [T(A,A,C)/(lam_2-lam_0) + T(B,B,C)/(lam_2-lam_1)]/2.
__global__ __launch_bounds__(256) void make_x4_jet_kernel(const float* __restrict__ x, const float* __restrict__ V,
                                                          int64_t n, int64_t npj, float* __restrict__ x4j) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < npj; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = c >> 4;
        const int li = (int)(c & 15);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (p < n) {
            if (li == 0) v = f32x4{x[p * 3], x[p * 3 + 1], x[p * 3 + 2], 1.f};
            else if (li <= 3) v = f32x4{V[p * 9 + li - 1], V[p * 9 + 3 + li - 1], V[p * 9 + 6 + li - 1], 0.f};
        }
        *reinterpret_cast<f32x4*>(x4j + c * 4) = v;
    }
}

__global__ __launch_bounds__(256) void curvature_kernel(const float* __restrict__ yj, const float* __restrict__ lam,
                                                        const float* __restrict__ V, int64_t n,
                                                        float* __restrict__ out_mean, float* __restrict__ out_gauss,
                                                        float* __restrict__ out_shape) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const float* yp = yj + p * 16;
        const double g0 = (double)lam[p * 3 + 2] - (double)lam[p * 3], g1 = (double)lam[p * 3 + 2] - (double)lam[p * 3 + 1];
        const double Taac = 2.0 * yp[10], Tbbc = 2.0 * yp[11], Tabc = yp[12], Tacc = 2.0 * yp[13], Tbcc = 2.0 * yp[14];
        if (out_mean) out_mean[p] = (float)(0.5 * (Taac / g0 + Tbbc / g1));
        if (out_shape || out_gauss) {
            double J[3][3], A[3], B[3], C[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { A[i] = V[p * 9 + i * 3]; B[i] = V[p * 9 + i * 3 + 1]; C[i] = V[p * 9 + i * 3 + 2]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double w0k = (A[k] * Taac + B[k] * Tabc + C[k] * Tacc) / g0;
                const double w1k = (A[k] * Tabc + B[k] * Tbbc + C[k] * Tbcc) / g1;
#pragma unroll
                for (int i = 0; i < 3; ++i) J[i][k] = A[i] * w0k + B[i] * w1k;
            }
            if (out_shape)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) out_shape[p * 9 + i * 3 + k] = (float)J[i][k];
            if (out_gauss) {
                // -det [[J, n], [n^T, 0]]  (reference src/render_st.py:48-53) = sum_ik n_i n_k cof(J)_ik
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
                        acc += C[i] * C[k] * (J[i1][k1] * J[i2][k2] - J[i1][k2] * J[i2][k1]);
                    }
                out_gauss[p] = (float)acc;
            }
        }
    }
}

// ---- sphere tracing on the device (reference src/render_st.py:136-172 `propagate_rays`, `grad_descent`) ----------------
// The reference keeps ray positions in float64 numpy, feeds float32 copies to the network, takes the step in float32
// (`inverse`, src/inverses.py:3-21) and adds it in float64.  Same here: t0 is double, x4 = (float)t0, the step float.
// 'squared' divides by the float64 sqrt(alpha) and rounds once, as the reference's in-place `/=` does (sqrt_alpha: host side).
__device__ __forceinline__ float inverse_step(float f, int inverse_mode, float alpha, double sqrt_alpha, float min_step) {
    if (inverse_mode == 0) return (f < 1.0f / alpha) ? sqrtf(f / alpha) : f;               // 'tanh'
    if (inverse_mode == 1) return (f > 0.f) ? f : min_step;                               // 'siren'
    return (float)((double)((f > 0.f) ? sqrtf(f) : min_step) / sqrt_alpha);               // 'squared'
}

__global__ __launch_bounds__(256) void rays_x4_kernel(const double* __restrict__ t0, int64_t m, int64_t np,
                                                      float* __restrict__ x4) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < np; p += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (p < m) v = f32x4{(float)t0[p * 3], (float)t0[p * 3 + 1], (float)t0[p * 3 + 2], 1.f};
        *reinterpret_cast<f32x4*>(x4 + p * 4) = v;
    }
}

// one marching iteration for the rays still active: step along the ray, record hits, retire rays (:141-156)
__global__ __launch_bounds__(256) void rays_step_kernel(const float* __restrict__ y, const double* __restrict__ rays,
                                                        double* __restrict__ t0, unsigned char* __restrict__ mask,
                                                        unsigned char* __restrict__ hits, int64_t m, int inverse_mode,
                                                        float alpha, double sqrt_alpha, float min_step, float threshold,
                                                        int* __restrict__ active) {
    int mine = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
        if (!mask[p]) continue;
        const float udf = y[p];
        const float step = inverse_step(fabsf(udf), inverse_mode, alpha, sqrt_alpha, min_step);
        double q[3];
        bool inside = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            q[k] = t0[p * 3 + k] + rays[p * 3 + k] * (double)step;
            t0[p * 3 + k] = q[k];
            inside = inside && q[k] > -1.0 && q[k] < 1.0;
        }
        const bool close = (inverse_mode == 1) ? (udf < threshold) : (fabsf(step) < threshold);
        if (close && inside) hits[p] = 1;
        const bool go_on = !close && inside;
        mask[p] = go_on ? 1 : 0;
        mine += go_on ? 1 : 0;
    }
    if (mine) atomicAdd(active, mine);
}

// one descent step for the hit rays: t0 -= normalize(grad f) * inverse(|f|)  (:163-172; src/util.py:35-40 `normalize`)
__global__ __launch_bounds__(256) void rays_descend_kernel(const float* __restrict__ y, const float* __restrict__ g,
                                                           double* __restrict__ t0, const unsigned char* __restrict__ hits,
                                                           int64_t m, int inverse_mode, float alpha, double sqrt_alpha,
                                                           float min_step) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
        if (!hits[p]) continue;
        const float gx = g[p * 4], gy = g[p * 4 + 1], gz = g[p * 4 + 2];
        const float nrm = sqrtf(gx * gx + gy * gy + gz * gz);
        const float step = inverse_step(fabsf(y[p]), inverse_mode, alpha, sqrt_alpha, min_step);
        t0[p * 3] -= (double)((gx / nrm) * step);
        t0[p * 3 + 1] -= (double)((gy / nrm) * step);
        t0[p * 3 + 2] -= (double)((gz / nrm) * step);
    }
}

constexpr int kGridCap = 2048;                         // workgroups per launch; the kernels stride over the rest

int dudf_launch_make_x4_jet(const float* x, const float* V, int64_t n, int64_t npj, float* x4j, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(make_x4_jet_kernel, dim3(dudf_grid_for(npj, 256, kGridCap)), dim3(256), 0, st, x, V, n, npj, x4j);
    return (int)hipGetLastError();
}

int dudf_launch_curvature(const float* yj, const float* lam, const float* V, int64_t n, float* out_mean,
                          float* out_gauss, float* out_shape, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(curvature_kernel, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), 0, st, yj, lam, V, n, out_mean,
                       out_gauss, out_shape);
    return (int)hipGetLastError();
}

int dudf_launch_rays_step(const DudfLayout& lo, const float* ws, const double* rays, double* t0, unsigned char* mask,
                          unsigned char* hits, int inverse_mode, double alpha, double min_step, double threshold,
                          int* active, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipError_t e = hipMemsetAsync(active, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(rays_step_kernel, dim3(dudf_grid_for(lo.n, 256, kGridCap)), dim3(256), 0, st, ws + lo.ws_y, rays, t0, mask,
                       hits, lo.n, inverse_mode, (float)alpha, sqrt(alpha), (float)min_step, (float)threshold, active);
    return (int)hipGetLastError();
}

int dudf_launch_rays_descend(const DudfLayout& lo, const float* ws, double* t0, const unsigned char* hits,
                             int inverse_mode, double alpha, double min_step, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(rays_descend_kernel, dim3(dudf_grid_for(lo.n, 256, kGridCap)), dim3(256), 0, st, ws + lo.ws_y, ws + lo.ws_g,
                       t0, hits, lo.n, inverse_mode, (float)alpha, sqrt(alpha), (float)min_step);
    return (int)hipGetLastError();
}

int dudf_launch_make_x4_grid(const DudfLayout& lo, int64_t grid_n, int64_t start, float* ws, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(make_x4_grid_kernel, dim3(dudf_grid_for(lo.np, 256, kGridCap)), dim3(256), 0, st, ws + lo.ws_x4, lo.n,
                       lo.np, grid_n, start);
    return (int)hipGetLastError();
}

// curvature query workspace = [Hessian-query layout of n points][lam 3n][V 9n][jet x4 4*npj][jet y npj]
struct CurvLayout { DudfLayout q; int64_t npj, o_lam, o_V, o_x4, o_y, o_relay; size_t total_bytes; };
int make_curv_layout(const dudf_net_cfg* cfg, int64_t n, CurvLayout* cl) {
    int rc = dudf_make_layout(cfg, n, n, &cl->q, 1);
    if (rc) return rc;
    cl->npj = (16 * n + DUDF_TILE_PTS - 1) / DUDF_TILE_PTS * DUDF_TILE_PTS;
    if (cl->npj == 0) cl->npj = DUDF_TILE_PTS;
    if (cl->npj > (1ll << 25)) return DUDF_E_BADCFG;
    DudfCarver cv = {(int64_t)(cl->q.total_bytes / sizeof(float))};
    cl->o_lam = cv.take(3 * n); cl->o_V = cv.take(9 * n); cl->o_x4 = cv.take(4 * cl->npj); cl->o_y = cv.take(cl->npj);
    // 512-wide layers: a layer's outputs reach the next one through memory (dudf_sweep_wide.hip, sweep_tile_w) — one layer's
    // worth of the jet columns, reused by every layer
    cl->o_relay = cl->q.H == 512 ? cv.take((int64_t)cl->q.H * cl->npj) : cl->o_y;
    cl->total_bytes = (size_t)cv.o * sizeof(float);
    return 0;
}

}  // namespace

int dudf_launch_copy_out(const DudfLayout& lo, const float* ws, float* out_f, float* out_g, float* out_h,
                         hipStream_t st) {
    hipLaunchKernelGGL(copy_out_kernel, dim3(dudf_grid_for(lo.n, 256, kGridCap)), dim3(256), 0, st, ws + lo.ws_y, ws + lo.ws_g,
                       out_f, out_g, out_h, lo.n, lo.n_h, lo.ncol_h);
    return (int)hipGetLastError();
}

int dudf_launch_rays_x4(const DudfLayout& lo, const double* t0, float* ws, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(rays_x4_kernel, dim3(dudf_grid_for(lo.np, 256, kGridCap)), dim3(256), 0, st, t0, lo.n, lo.np, ws + lo.ws_x4);
    return (int)hipGetLastError();
}

int dudf_launch_field_features(const DudfLayout& lo, const float* ws, int inverse_mode, double alpha, float* out_df,
                               float* out_vec, int* out_flag_count, float* out_lam, float* out_V, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    if (out_flag_count) {
        hipError_t e = hipMemsetAsync(out_flag_count, 0, sizeof(int), st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(field_features_kernel, dim3(dudf_grid_for(lo.n, 256, kGridCap)), dim3(256), 0, st, ws + lo.ws_y,
                       ws + lo.ws_g, lo.n, lo.n_h, lo.ncol_h, inverse_mode, (float)alpha, sqrt(alpha), out_df, out_vec, out_flag_count,
                       out_lam,
                       out_V);
    return (int)hipGetLastError();
}

extern "C" {

int dudf_query(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f, float* out_g,
               void* workspace, size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = dudf_forward_common(c, theta, x, 0, out_g != nullptr))) return rc;
    return dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, nullptr, c.st);
}

int dudf_query_hessian(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f,
                       float* out_g, float* out_h, void* workspace, size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, n, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = dudf_forward_common(c, theta, x, 0, true))) return rc;
    return dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, out_h, c.st);
}

int dudf_query_frame(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f,
                     float* out_g, float* out_h, float* out_lambda, float* out_v, void* workspace,
                     size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, n, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = dudf_forward_common(c, theta, x, 0, true))) return rc;
    if ((rc = dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, out_h, c.st))) return rc;
    return dudf_launch_field_features(c.lo, c.ws, 0, 1.0, nullptr, nullptr, nullptr, out_lambda, out_v, c.st);
}

size_t dudf_workspace_bytes_curvature(const dudf_net_cfg* cfg, int64_t n) {
    CurvLayout cl;
    if (make_curv_layout(cfg, n, &cl)) return 0;
    return cl.total_bytes;
}

int dudf_query_curvature(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
                         float* out_lambda, float* out_v, float* out_mean, float* out_gauss, float* out_shape,
                         void* workspace, size_t workspace_bytes, void* stream) {
    CurvLayout cl;
    int rc = make_curv_layout(cfg, n, &cl);
    if (rc) return rc;
    // (the column limit of a query layout, 2^25, cannot be what stops this call: the 16 jet columns per point reach it first)
    if ((rc = dudf_check_buffer(workspace, workspace_bytes, cl.total_bytes))) return rc;
    if (n <= 0) return 0;
    DudfCtx c = dudf_ctx_at(cl.q, reinterpret_cast<float*>(workspace), reinterpret_cast<hipStream_t>(stream));
    // 1. value, df/dx, Hessian (forward-over-reverse quads) and the eigen-frame of the Hessian
    if ((rc = dudf_forward_common(c, theta, x, 0, true))) return rc;
    float* lam = c.ws + cl.o_lam; float* V = c.ws + cl.o_V;
    if ((rc = dudf_launch_field_features(c.lo, c.ws, 0, 1.0, nullptr, nullptr, nullptr, lam, V, c.st))) return rc;
    // 2. third-order Taylor jet in the three frame directions: one 16-column tile per point
    if ((rc = dudf_launch_make_x4_jet(x, V, n, cl.npj, c.ws + cl.o_x4, c.st))) return rc;
    SweepArgs a = dudf_make_sweep_args(c.lo, theta, c.ws);
    a.x4 = c.ws + cl.o_x4; a.y = c.ws + cl.o_y; a.np = cl.npj; a.stash_layer = (int64_t)c.lo.H * cl.npj;
    if (c.lo.H == 512) { a.S = c.ws + cl.o_relay; a.stash_layer = 0; }     // every layer's slot is the same one
    a.tile0 = 0; a.ntiles = (int)(cl.npj / DUDF_TILE_PTS); a.hess = 1;
    if ((rc = dudf_launch_range(SWEEP_FWD_J, c.lo.H, a, c.st))) return rc;
    // 3. first-order eigenvector perturbation
    if ((rc = dudf_launch_curvature(c.ws + cl.o_y, lam, V, n, out_mean, out_gauss, out_shape, c.st))) return rc;
    hipError_t e = hipSuccess;
    if (out_lambda) e = hipMemcpyAsync(out_lambda, lam, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c.st);
    if (e == hipSuccess && out_v) e = hipMemcpyAsync(out_v, V, (size_t)n * 9 * sizeof(float), hipMemcpyDeviceToDevice, c.st);
    return (int)e;
}

int dudf_grid_fields(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int64_t start, int64_t count,
                     int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (grid_n < 2 || start < 0 || count < 0 || start + count > grid_n * grid_n * grid_n) return DUDF_E_BADCFG;
    if (!dudf_valid_inverse_mode(inverse_mode)) return DUDF_E_BADMODE;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, count, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (count == 0) return 0;
    if ((rc = dudf_launch_make_x4_grid(c.lo, grid_n, start, c.ws, c.st))) return rc;
    if ((rc = dudf_forward_common(c, theta, nullptr, 0, true))) return rc;
    return dudf_launch_field_features(c.lo, c.ws, inverse_mode, alpha, out_df, out_vec, out_flag_count, nullptr,
                                      nullptr, c.st);
}

int dudf_grid_values(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int64_t start, int64_t count, float* out_f,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (grid_n < 2 || start < 0 || count < 0 || start + count > grid_n * grid_n * grid_n) return DUDF_E_BADCFG;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, count, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (count == 0) return 0;
    if ((rc = dudf_launch_make_x4_grid(c.lo, grid_n, start, c.ws, c.st))) return rc;
    if ((rc = dudf_forward_common(c, theta, nullptr, 0, false))) return rc;      // value only: no reverse sweep
    return dudf_launch_copy_out(c.lo, c.ws, out_f, nullptr, nullptr, c.st);
}

int dudf_trace_rays(const dudf_net_cfg* cfg, const float* theta, const double* rays, double* t0, unsigned char* mask,
                    unsigned char* hits, int64_t m, int inverse_mode, double alpha, double min_step,
                    double surface_threshold, int max_iterations, int check_every, int* iterations_done,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!dudf_valid_inverse_mode(inverse_mode) || max_iterations < 0 || check_every < 1) return DUDF_E_BADMODE;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, m, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (iterations_done) *iterations_done = 0;
    if (m <= 0) return 0;
    hipError_t e = hipMemsetAsync(hits, 0, (size_t)m, c.st);
    if (e != hipSuccess) return (int)e;
    if ((rc = dudf_launch_pack(c.lo, theta, c.ws, c.st))) return rc;
    if (dudf_use_bf16_sweeps() && (rc = dudf_launch_pack_bf16(c.lo, theta, c.ws, c.st))) return rc;
    SweepArgs a = dudf_make_sweep_args(c.lo, theta, c.ws);
    int* active = reinterpret_cast<int*>(c.ws + c.lo.ws_acc);
    int it = 0;
    for (; it < max_iterations; ++it) {
        // value-only queries at the current positions of ALL rays (retired ones are evaluated and ignored: no compaction,
        // no per-iteration host round trip), then the step / hit / retire update of the active ones
        if ((rc = dudf_launch_rays_x4(c.lo, t0, c.ws, c.st))) return rc;
        if ((rc = dudf_run_sweep(SWEEP_FWD, c.lo, a, c.st))) return rc;
        if ((rc = dudf_launch_rays_step(c.lo, c.ws, rays, t0, mask, hits, inverse_mode, alpha, min_step, surface_threshold,
                                        active, c.st))) return rc;
        if ((it + 1) % check_every == 0 || it + 1 == max_iterations) {   // the reference's `while np.sum(mask_rays) > 0`
            int left = 0;
            if ((e = hipMemcpyAsync(&left, active, sizeof(int), hipMemcpyDeviceToHost, c.st)) != hipSuccess) return (int)e;
            if ((e = hipStreamSynchronize(c.st)) != hipSuccess) return (int)e;
            if (left == 0) { ++it; break; }
        }
    }
    if (iterations_done) *iterations_done = it;
    return 0;
}

int dudf_descend_rays(const dudf_net_cfg* cfg, const float* theta, double* t0, const unsigned char* hits, int64_t m,
                      int inverse_mode, double alpha, double min_step, int gd_steps, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!dudf_valid_inverse_mode(inverse_mode) || gd_steps < 0) return DUDF_E_BADMODE;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, m, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (m <= 0) return 0;
    for (int s = 0; s < gd_steps; ++s) {
        if ((rc = dudf_launch_rays_x4(c.lo, t0, c.ws, c.st))) return rc;
        if ((rc = dudf_forward_common(c, theta, nullptr, 0, true))) return rc;
        if ((rc = dudf_launch_rays_descend(c.lo, c.ws, t0, hits, inverse_mode, alpha, min_step, c.st))) return rc;
    }
    return 0;
}

}  // extern "C"
