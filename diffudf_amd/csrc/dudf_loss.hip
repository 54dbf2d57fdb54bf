// The training step's small kernels: parameter packing, the per-point loss terms and their cotangents, loss_s2
// statistics, x4, copy-in, Adam, stash reads; with their launchers.  All bandwidth-trivial.
#include "dudf_internal.h"
#include "dudf_eigh3.h"

namespace {

// ---- pack: A-operand forms of theta --------------------------------------------------------------
__global__ void pack_kernel(const float* __restrict__ theta, float* __restrict__ w1b, float* __restrict__ b1s, float* __restrict__ w1t16,
                            float* __restrict__ wt, int H, int L, int64_t off_hid, int64_t hid_stride, float rho) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_wt = (int64_t)(L - 1) * H * H;
    if (gid < n_wt) {                                   // wt[j][i][o] = W_{j+2}[o][i]
        const int64_t j = gid / ((int64_t)H * H), rem = gid % ((int64_t)H * H);
        const int i = (int)(rem / H), o = (int)(rem % H);
        wt[gid] = theta[off_hid + j * hid_stride + (int64_t)o * H + i];
    }
    if (gid < 4 * (int64_t)H) {                         // w1b[f][k] = k<3 ? W_1[f][k] : b_1[f]
        const int f = (int)(gid / 4), k = (int)(gid % 4);
        w1b[gid] = rho * (k < 3 ? theta[f * 3 + k] : theta[3 * H + f]);
        if (k == 3) b1s[f] = rho * theta[3 * H + f];
    }
    if (gid >= H && gid < (int64_t)L * H) {             // b1s rows 1 .. L-1 = b_2 .. b_L
        const int layer = (int)(gid / H), f = (int)(gid % H);
        b1s[gid] = theta[off_hid + (int64_t)(layer - 1) * hid_stride + (int64_t)H * H + f];
    }
    if (gid < 16 * (int64_t)H) {                        // w1t16[r][f] = r<3 ? W_1[f][r] : 0
        const int r = (int)(gid / H), f = (int)(gid % H);
        w1t16[gid] = r < 3 ? rho * theta[f * 3 + r] : 0.f;
    }
}

// ---- reductions ---------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NV>
__device__ __forceinline__ void block_accumulate(double (&v)[NV], double* __restrict__ acc) {
    __shared__ double part[NV][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum_d(v[i]);
        if (lane == 0) part[i][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const double s = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        atomicAdd(acc + threadIdx.x, s);
    }
}

struct LossArgs {
    const float *y, *g, *normals, *sdf;     // y [np], g [np][4] per COLUMN; normals (n,3), sdf (n) per POINT
    float *ybar, *gbar;                      // per column
    const float* cot;                        // device, 4 floats
    const double* stats;                     // device, 3 doubles (s2)
    double* acc;                             // device, >= 4 doubles (+ one ticket word behind them)
    int64_t n, n_h, ncol_h, np, ncols;
    float w[4];
    float alpha, inv_n;                      // 1 / n_global
    // loss_fwd: the last block to finish turns the four sums into the four weighted terms (no second launch)
    float* out_terms; double wd[4]; double inv_nd;
    // loss_bwd: buffers this kernel zeroes on its way (d(theta) before the weight-gradient atomics, the running maxima of
    // A_l / zbar_l before the adjoint sweeps) instead of two memset launches
    float* zero_f; int64_t zero_fn; unsigned* zero_u; int zero_un;
};

__device__ __forceinline__ int64_t col_of(const LossArgs& a, int64_t p) {
    return p < a.n_h ? 4 * p : a.ncol_h + (p - a.n_h);
}

__device__ __forceinline__ float sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }

// per-point pieces of loss_s1 (reference src/loss_functions.py:131-136, :9-22)
__device__ __forceinline__ void s1_point(float y, const f32x4 g, float u, float alpha,
                                         float& t_on, float& t_off, float& t_g, float& tdf, float& gn, float& tau) {
    const float tn = tanhf(alpha * u);
    tdf = u * tn;
    const bool on = (u == 0.f);
    t_on = on ? fabsf(y) : 0.f;
    t_off = on ? 0.f : fabsf(tdf - y);
    gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    tau = fabsf(tn + u * alpha * (1.f - tn * tn));
    t_g = fabsf(gn - tau);
}

// Hessian of a quad: H[i][k] = (adot_0^k)_i = g[(4p+1+k)*4 + i]
__device__ __forceinline__ void load_hessian(const LossArgs& a, int64_t p, double (&Hm)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f32x4 col = *reinterpret_cast<const f32x4*>(a.g + (4 * p + 1 + k) * 4);
        Hm[0][k] = col[0]; Hm[1][k] = col[1]; Hm[2][k] = col[2];
    }
}

// (1 - |cos(m, n)|) for the top eigenvector n, and (when wanted) the cotangent of H for an upstream factor k2
// on that term (reference principal_curvature_alignment :45-53 + eigh backward)
__device__ __forceinline__ float hess_term(const LossArgs& a, int64_t p, const float* m3, double k2, bool want_bar,
                                           double (&Hb)[3][3]) {
    double Hm[3][3], lam[3], V[3][3];
    load_hessian(a, p, Hm);
    eigh3(Hm, lam, V);
    const double m[3] = {m3[0], m3[1], m3[2]};
    const double n[3] = {V[0][2], V[1][2], V[2][2]};
    const double mn = fmax(sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), 1e-8);
    const double nn = fmax(sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-8);
    const double cs = (m[0] * n[0] + m[1] * n[1] + m[2] * n[2]) / (mn * nn);
    if (want_bar) {
        const double sg = (cs > 0) ? 1.0 : ((cs < 0) ? -1.0 : 0.0);
        double nb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) nb[i] = -k2 * sg * (m[i] / (mn * nn) - cs * n[i] / (nn * nn));
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) Hb[i][k] = 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double vj[3] = {V[0][j], V[1][j], V[2][j]};
            const double coef = 0.5 * (vj[0] * nb[0] + vj[1] * nb[1] + vj[2] * nb[2]) / (lam[2] - lam[j]);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) Hb[i][k] += coef * (vj[i] * n[k] + n[i] * vj[k]);
        }
    }
    return (float)(1.0 - fabs(cs));
}

// mode 0: loss_s1, mode 2: loss_siren (reference :82-104, :24-32)
template <int MODE>
__global__ __launch_bounds__(256) void loss_fwd_kernel(LossArgs a) {
    double v[4] = {0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = col_of(a, p);
        const float y = a.y[c];
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.g + c * 4);
        const float u = a.sdf[p];
        if constexpr (MODE == DUDF_LOSS_S1) {
            float t_on, t_off, t_g, tdf, gn, tau;
            s1_point(y, g, u, a.alpha, t_on, t_off, t_g, tdf, gn, tau);
            v[0] += t_on; v[1] += t_off;
            if (a.w[3] != 0.f) v[3] += t_g;
            if (a.w[2] != 0.f) {
                // the Hessian path is a property of the LAYOUT (the first n_hess points carry quads), the term one of the
                // DATA (sdf == 0): a batch whose on-surface points are not exactly the leading n_hess would train on a
                // Hessian term over the wrong points — the term (and, below, the gradient) turn NaN instead
                if ((p < a.n_h) != (u == 0.f)) v[2] += __builtin_nan("");
                else if (p < a.n_h) {
                    double Hb[3][3];
                    v[2] += hess_term(a, p, a.normals + p * 3, 0.0, false, Hb);
                }
            }
        } else {
            const bool on = (u == 0.f);
            const float ay = fabsf(y);
            const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
            v[0] += on ? ay : 0.f;
            v[1] += on ? 0.f : expf(-100.f * ay);
            if (on) {
                const float m0 = a.normals[p * 3], m1 = a.normals[p * 3 + 1], m2 = a.normals[p * 3 + 2];
                const float mn = sqrtf(m0 * m0 + m1 * m1 + m2 * m2);
                const float cs = (g[0] * m0 + g[1] * m1 + g[2] * m2) / (fmaxf(gn, 1e-8f) * fmaxf(mn, 1e-8f));
                v[2] += 1.f - cs;
            }
            v[3] += (gn - 1.f) * (gn - 1.f);
        }
    }
    block_accumulate<4>(v, a.acc);
    // last block done: finalize.  (The atomics above are device-scope; the fence orders them before the ticket.)
    __shared__ bool last;
    __threadfence();
    if (threadIdx.x == 0) {
        unsigned* ticket = reinterpret_cast<unsigned*>(a.acc + 4);
        last = (atomicAdd(ticket, 1u) == gridDim.x - 1);
    }
    __syncthreads();
    if (last && threadIdx.x < 4) {
        __threadfence();
        const double sum = atomicAdd(a.acc + threadIdx.x, 0.0);       // read through the atomic path: every block's add is visible
        // loss_s1: a NaN Hessian term (a batch that breaks the n_hess layout, above) takes every term with it — the sum the
        // loop backpropagates is NaN either way, and a log that shows three healthy numbers next to it would mislead
        const bool poisoned = MODE == DUDF_LOSS_S1 && a.w[2] != 0.f && isnan(atomicAdd(a.acc + 2, 0.0));
        a.out_terms[threadIdx.x] = poisoned ? __builtin_nanf("") : (float)(sum * a.inv_nd * a.wd[threadIdx.x]);
    }
}

__global__ void loss_finalize_kernel(const double* acc, float* out, double w0, double w1, double w2, double w3,
                                     double inv_n) {
    if (threadIdx.x == 0) {
        out[0] = (float)(acc[0] * inv_n * w0);
        out[1] = (float)(acc[1] * inv_n * w1);
        out[2] = (float)(acc[2] * inv_n * w2);
        out[3] = (float)(acc[3] * inv_n * w3);
    }
}

// cotangents ybar (on y) and gbar (on the a_0 rows: df/dx, and for Hessian quads the three Hessian columns) of
// sum_i cot[i] * term_i   (SURVEY.md Appendix A.4).  One thread per UNIT = one plain column or one whole quad;
// padded columns get zeros.
template <int MODE>
__global__ __launch_bounds__(256) void loss_bwd_kernel(LossArgs a) {
    const float c0 = a.cot[0], c1 = a.cot[1], c2 = (MODE == DUDF_LOSS_S2) ? 0.f : a.cot[2],
                c3 = (MODE == DUDF_LOSS_S2) ? 0.f : a.cot[3];
    double mu = 0, sd = 1, cnt = 2;
    if constexpr (MODE == DUDF_LOSS_S2) {
        cnt = a.stats[0];
        mu = a.stats[1] / cnt;
        sd = sqrt((a.stats[2] - cnt * mu * mu) / (cnt - 1.0));
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.zero_fn; i += (int64_t)gridDim.x * blockDim.x) a.zero_f[i] = 0.f;
    if (blockIdx.x == 0 && (int)threadIdx.x < a.zero_un) a.zero_u[threadIdx.x] = 0u;
    const int64_t nq = a.ncol_h / 4;                                   // quads (padded)
    const int64_t units = nq + (a.ncols - a.ncol_h);
    for (int64_t uidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; uidx < units;
         uidx += (int64_t)gridDim.x * blockDim.x) {
        const bool quad = uidx < nq;
        const int64_t p = quad ? uidx : a.n_h + (uidx - nq);
        const int64_t c = quad ? 4 * uidx : a.ncol_h + (uidx - nq);
        const bool valid = quad ? (p < a.n_h) : (p < a.n);
        float yb = 0.f;
        f32x4 gb = {0, 0, 0, 0};
        double Hb[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        if (valid) {
            const float y = a.y[c];
            const float u = a.sdf[p];
            const bool on = (u == 0.f);
            if constexpr (MODE == DUDF_LOSS_S1) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(a.g + c * 4);
                float t_on, t_off, t_g, tdf, gn, tau;
                s1_point(y, g, u, a.alpha, t_on, t_off, t_g, tdf, gn, tau);
                yb = on ? c0 * a.w[0] * a.inv_n * sgn(y) : -c1 * a.w[1] * a.inv_n * sgn(tdf - y);
                if (a.w[3] != 0.f && gn > 0.f) {
                    const float k = c3 * a.w[3] * a.inv_n * sgn(gn - tau) / gn;
                    gb = f32x4{k * g[0], k * g[1], k * g[2], 0.f};
                }
                if (a.w[2] != 0.f) {
                    if (quad != on) yb = __builtin_nanf("");          // wrong n_hess for this batch (see loss_fwd_kernel): loud
                    else if (quad) hess_term(a, p, a.normals + p * 3, (double)c2 * a.w[2] * a.inv_n, true, Hb);
                }
            } else if constexpr (MODE == DUDF_LOSS_SIREN) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(a.g + c * 4);
                const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                yb = on ? c0 * a.w[0] * a.inv_n * sgn(y)
                        : -c1 * a.w[1] * a.inv_n * 100.f * sgn(y) * expf(-100.f * fabsf(y));
                float k = (gn > 0.f) ? c3 * a.w[3] * a.inv_n * 2.f * (gn - 1.f) / gn : 0.f;
                gb = f32x4{k * g[0], k * g[1], k * g[2], 0.f};
                if (on) {
                    // d cos / d g = k1 m - k2 g in double, rounded once: where g is parallel to the normal — the state this term
                    // trains towards — the two products cancel, and fp32 left 1e-7 of k1 |m| standing in place of a cotangent
                    // that is zero: 1.6e-5 of the point's largest cotangent (tests/test_loss_stage_gpu.py)
                    const double m[3] = {a.normals[p * 3], a.normals[p * 3 + 1], a.normals[p * 3 + 2]};
                    const double gd[3] = {g[0], g[1], g[2]};
                    const double gnd = sqrt(gd[0] * gd[0] + gd[1] * gd[1] + gd[2] * gd[2]);
                    const double mnd = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
                    const double gnc = fmax(gnd, 1e-8), mnc = fmax(mnd, 1e-8);
                    const double cs = (gd[0] * m[0] + gd[1] * m[1] + gd[2] * m[2]) / (gnc * mnc);
                    const double ka = -(double)c2 * a.w[2] * a.inv_n;
                    const double k1 = ka / (gnc * mnc);
                    const double k2 = (gnd > 1e-8) ? ka * cs / (gnc * gnc) : 0.0;
#pragma unroll
                    for (int i = 0; i < 3; ++i) gb[i] += (float)(k1 * m[i] - k2 * gd[i]);
                }
            } else {                                     // loss_s2 (reference :106-121)
                if (on) {
                    const double smu = (mu > 0) ? 1.0 : ((mu < 0) ? -1.0 : 0.0);
                    yb = (float)((double)c0 * a.w[0] * smu / cnt + (double)c1 * a.w[1] * ((double)y - mu) / ((cnt - 1.0) * sd));
                }
            }
        }
        a.ybar[c] = yb;
        *reinterpret_cast<f32x4*>(a.gbar + c * 4) = gb;
        if (quad) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {                // cotangent of adot_0^k = column k of Hbar
                a.ybar[c + 1 + k] = 0.f;
                *reinterpret_cast<f32x4*>(a.gbar + (c + 1 + k) * 4) =
                    f32x4{(float)Hb[0][k], (float)Hb[1][k], (float)Hb[2][k], 0.f};
            }
        }
    }
}

__global__ __launch_bounds__(256) void s2_stats_kernel(LossArgs a, double* __restrict__ stats) {
    double v[3] = {0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * blockDim.x) {
        if (a.sdf[p] == 0.f) {
            const double yy = a.y[col_of(a, p)];
            v[0] += 1.0; v[1] += yy; v[2] += yy * yy;
        }
    }
    block_accumulate<3>(v, stats);
}

__global__ void s2_terms_kernel(const double* stats, double w0, double w1, float* out) {
    if (threadIdx.x == 0) {
        const double cnt = stats[0], mu = stats[1] / cnt;
        const double var = (stats[2] - cnt * mu * mu) / (cnt - 1.0);
        out[0] = (float)(fabs(mu) * w0);
        // a cancellation residue below zero is zero; the NaN of fewer than two on-surface points (0 / 0) stays one, as torch.std's
        // does (reference :115) — `var > 0 ? var : 0.0` reported a std of 0 for a batch whose backward is NaN
        out[1] = (float)(sqrt(var < 0 ? 0.0 : var) * w1);
    }
}

// x4: the layer-1 B operand of every column.  plain column: (x0,x1,x2,1) — the 1 multiplies the bias column of
// [W_1|b_1]; Hessian quad: channel 0 the same, channel 1+k = (e_k, 0) (hdot_0^k = e_k, no bias); padding: zeros.
__global__ __launch_bounds__(256) void make_x4_kernel(const float* __restrict__ x, float* __restrict__ x4, int64_t n,
                                                      int64_t n_h, int64_t ncol_h, int64_t np) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < np; c += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = {0, 0, 0, 0};
        if (c < ncol_h) {
            const int64_t p = c >> 2; const int ch = (int)(c & 3);
            if (p < n_h) {
                if (ch == 0) v = f32x4{x[p * 3], x[p * 3 + 1], x[p * 3 + 2], 1.f};
                else v[ch - 1] = 1.f;
            }
        } else {
            const int64_t p = n_h + (c - ncol_h);
            if (p < n) v = f32x4{x[p * 3], x[p * 3 + 1], x[p * 3 + 2], 1.f};
        }
        *reinterpret_cast<f32x4*>(x4 + c * 4) = v;
    }
}

// ---- Adam (torch.optim.Adam single-tensor semantics, reference train.py:334-337) -------------------
// Operation by operation what torch's CUDA Adam executes (torch/optim/adam.py _multi_tensor_adam: lerp_, mul_, addcmul_,
// sqrt, div_, add_, addcdiv_), with the SAME constants: 1 - beta are formed in double on the host and rounded once
// (1.f - 0.999f in float is off by 1.3e-5 relative, which moved the second moment and, over a dozen steps, the loss
// curve by 1e-5).  Each torch kernel rounds its result to fp32; inside one kernel clang contracts a*b + c, as it does here.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ theta, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   float w1, float b2, float w2, float eps, float step_size,
                                                   float bc2_sqrt, float gscale) {
#pragma clang fp contract(off)                                   // only the fmaf below fuse (HIP's __fmul_rn etc. are plain operators)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gscale;
        const float mi = fmaf(w1, gi - m[i], m[i]);               // lerp_(grad, 1 - beta1), weight < 0.5 branch
        const float vs = __fmul_rn(v[i], b2);                      // mul_(beta2)
        const float vi = fmaf(__fmul_rn(w2, gi), gi, vs);          // addcmul_(grad, grad, value = 1 - beta2)
        m[i] = mi; v[i] = vi;
        const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vi), bc2_sqrt), eps);
        theta[i] = fmaf(-step_size, __fdiv_rn(mi, denom), theta[i]);   // addcdiv_(exp_avg, denom, value = -step_size)
    }
}

// The same update with (step_size, bc2_sqrt) taken from row *row of a device table (dudf_adam_step_scheduled: the form a captured
// HIP graph replays).  The arithmetic is adam_kernel's, statement for statement.
__global__ __launch_bounds__(256) void adam_sched_kernel(float* __restrict__ theta, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                         float w1, float b2, float w2, float eps,
                                                         const float* __restrict__ sched, int64_t n_rows,
                                                         const int64_t* __restrict__ row, float gscale) {
#pragma clang fp contract(off)
    const int64_t r = *row;
    const bool bad = r < 0 || r >= n_rows;
    const float step_size = bad ? 0.f : sched[2 * r], bc2_sqrt = bad ? 1.f : sched[2 * r + 1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (bad) { theta[i] = __builtin_nanf(""); continue; }      // past the end of the schedule: loud, not silent
        const float gi = g[i] * gscale;
        const float mi = fmaf(w1, gi - m[i], m[i]);
        const float vs = __fmul_rn(v[i], b2);
        const float vi = fmaf(__fmul_rn(w2, gi), gi, vs);
        m[i] = mi; v[i] = vi;
        const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vi), bc2_sqrt), eps);
        theta[i] = fmaf(-step_size, __fdiv_rn(mi, denom), theta[i]);
    }
}

__global__ __launch_bounds__(256) void read_stash_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                         int64_t n, int64_t n_h, int64_t ncol_h, int64_t np, int H,
                                                         int channel, int per_quad, int p24, const float* __restrict__ fx) {
    const int64_t tot = n * H;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i / H; const int f = (int)(i % H);
        // Hessian-path points: four columns (channels) per point — except in C, which keeps one copy per quad (LaneOff)
        const int64_t c = p < n_h ? (per_quad ? p : 4 * p + channel) : ncol_h + (p - n_h);
        if (p24) {
            // 24-bit tile-major array (dudf_internal.h): granule of (feature quad, column) = 3 dwords holding the top three
            // bytes of four values; `src` already points at the layer (H * np * 3 bytes per layer)
            const unsigned* g = reinterpret_cast<const unsigned*>(src) +
                                ((((int64_t)(f >> 4) * (np >> 4) + (c >> 4)) * 64) + 16 * ((f & 15) >> 2) + (c & 15)) * 3;
            const unsigned d0 = g[0], d1 = g[1], d2 = g[2];
            const int e = f & 3;
            if (p24 == 2) {                                  // C: fixed point — the low 24 bits of bits(c + 3.0f) (c24_pack)
                const unsigned u = e == 0 ? d0 & 0xffffffu : e == 1 ? d1 & 0xffffffu : e == 2 ? d2 & 0xffffffu
                                                                  : (d0 >> 24) | ((d1 >> 24) << 8) | ((d2 >> 24) << 16);
                out[i] = __uint_as_float(0x40000000u | u) - 3.0f;
            } else if (p24 == 3) {                           // S, Q, A, Z: the same fixed point, times the column's 2^E (fx: this layer's row)
                const unsigned u = e == 0 ? d0 & 0xffffffu : e == 1 ? d1 & 0xffffffu : e == 2 ? d2 & 0xffffffu
                                                                  : (d0 >> 24) | ((d1 >> 24) << 8) | ((d2 >> 24) << 16);
                out[i] = (__uint_as_float(0x40000000u | u) - 3.0f) * fx[c];
            } else {
                const unsigned u = e == 0 ? d0 << 8 : e == 1 ? ((d0 >> 24) << 8) | (d1 << 16) : e == 2 ? ((d1 >> 16) << 8) | (d2 << 24) : d2 & 0xffffff00u;
                out[i] = __uint_as_float(u);
            }
        } else {
            out[i] = src[((int64_t)(f >> 2) * np + c) * 4 + (f & 3)];
        }
    }
}

// ybar (n) / gbar (n,3) given per POINT by the caller -> per column (tangent channels and padding zero)
__global__ __launch_bounds__(256) void copy_in_kernel(const float* __restrict__ ybar, const float* __restrict__ gbar,
                                                      float* __restrict__ wy, float* __restrict__ wg, int64_t n,
                                                      int64_t n_h, int64_t ncol_h, int64_t np) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < np; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = -1;
        if (c < ncol_h) { if ((c & 3) == 0 && (c >> 2) < n_h) p = c >> 2; }
        else if (n_h + (c - ncol_h) < n) p = n_h + (c - ncol_h);
        wy[c] = (p >= 0 && ybar) ? ybar[p] : 0.f;
        f32x4 gv = {0, 0, 0, 0};
        if (p >= 0 && gbar) gv = f32x4{gbar[p * 3], gbar[p * 3 + 1], gbar[p * 3 + 2], 0.f};
        *reinterpret_cast<f32x4*>(wg + c * 4) = gv;
    }
}

constexpr int kGridCap = 2048;                         // workgroups per launch; the kernels stride over the rest

LossArgs make_loss_args(const DudfLayout& lo, const float* normals, const float* sdf, int64_t n_global,
                        const double* w, double alpha, float* ws) {
    LossArgs a;
    a.y = ws + lo.ws_y; a.g = ws + lo.ws_g; a.normals = normals; a.sdf = sdf;
    a.ybar = ws + lo.ws_ybar; a.gbar = ws + lo.ws_gbar; a.cot = nullptr; a.stats = nullptr;
    a.acc = reinterpret_cast<double*>(ws + lo.ws_acc);
    a.n = lo.n; a.n_h = lo.n_h; a.ncol_h = lo.ncol_h; a.np = lo.np; a.ncols = lo.ncols;
    for (int i = 0; i < 4; ++i) a.w[i] = (float)w[i];
    a.alpha = (float)alpha; a.inv_n = (float)(1.0 / (double)n_global);
    a.out_terms = nullptr; a.inv_nd = 0.0; a.wd[0] = a.wd[1] = a.wd[2] = a.wd[3] = 0.0;
    a.zero_f = nullptr; a.zero_fn = 0; a.zero_u = nullptr; a.zero_un = 0;
    return a;
}

}  // namespace

int dudf_launch_pack(const DudfLayout& lo, const float* theta, float* ws, hipStream_t st) {
    DudfProfScope prof(PROF_PACK, st);
    int64_t n = (int64_t)(lo.L - 1) * lo.H * lo.H;
    if (n < 16 * (int64_t)lo.H) n = 16 * (int64_t)lo.H;
    if (n < (int64_t)lo.L * lo.H) n = (int64_t)lo.L * lo.H;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, theta, ws + lo.ws_w1b, ws + lo.ws_b1s,
                       ws + lo.ws_w1t16, ws + lo.ws_wt, lo.H, lo.L, lo.off_hid, lo.hid_stride, lo.rho);
    return (int)hipGetLastError();
}

int dudf_launch_loss_fwd(const DudfLayout& lo, int mode, const float* normals, const float* sdf, int64_t n_global,
                         const double* w, double alpha, float* ws, float* out_terms, hipStream_t st) {
    DudfProfScope prof(PROF_LOSS_FWD, st);
    LossArgs a = make_loss_args(lo, normals, sdf, n_global, w, alpha, ws);
    // (the four sums and the ticket behind them were zeroed by the forward's prep kernel, dudf_launch_prep)
    a.out_terms = out_terms; a.inv_nd = 1.0 / (double)n_global;
    for (int i = 0; i < 4; ++i) a.wd[i] = w[i];
    // deterministic mode: one block = one fixed summation order.  Otherwise every block ends in four fp64 atomics on the SAME
    // four addresses: at 391 blocks (100 000 points) the kernel spent 30 us queueing them; without the Hessian term a point
    // costs a few dozen flops, so 128 blocks with a grid-stride loop finish sooner.  (With it — an fp64 Jacobi eigensolve per
    // on-surface point — the work dominates: as many blocks as there are points for.)
    int grid = dudf_deterministic() ? 1 : dudf_grid_for(lo.n, 256, kGridCap);
    if (!dudf_deterministic() && !(mode == DUDF_LOSS_S1 && w[2] != 0.0 && lo.n_h > 0) && grid > 128) grid = 128;
    if (mode == DUDF_LOSS_S1) hipLaunchKernelGGL(loss_fwd_kernel<DUDF_LOSS_S1>, dim3(grid), dim3(256), 0, st, a);
    else if (mode == DUDF_LOSS_SIREN) hipLaunchKernelGGL(loss_fwd_kernel<DUDF_LOSS_SIREN>, dim3(grid), dim3(256), 0, st, a);
    else return DUDF_E_BADMODE;
    return (int)hipGetLastError();
}

int dudf_launch_loss_bwd(const DudfLayout& lo, int mode, const float* normals, const float* sdf, int64_t n_global,
                         const double* w, double alpha, const float* cot, const double* stats, float* ws,
                         hipStream_t st, float* zero_f, int64_t zero_fn) {
    DudfProfScope prof(PROF_LOSS_BWD, st);
    LossArgs a = make_loss_args(lo, normals, sdf, n_global, w, alpha, ws);
    a.cot = cot; a.stats = stats;
    a.zero_f = zero_f; a.zero_fn = zero_f ? zero_fn : 0;
    // a backward may run several times per forward: the running maxima of A_l and zbar_l (rows 1, 2 of amax) start over
    a.zero_u = reinterpret_cast<unsigned*>(ws + lo.ws_amax) + lo.L; a.zero_un = (dudf_split_fp16() && 2 * lo.L <= 256) ? 2 * lo.L : 0;
    const int grid = dudf_grid_for(lo.np, 256, kGridCap);
    if (mode == DUDF_LOSS_S1) hipLaunchKernelGGL(loss_bwd_kernel<DUDF_LOSS_S1>, dim3(grid), dim3(256), 0, st, a);
    else if (mode == DUDF_LOSS_SIREN) hipLaunchKernelGGL(loss_bwd_kernel<DUDF_LOSS_SIREN>, dim3(grid), dim3(256), 0, st, a);
    else if (mode == DUDF_LOSS_S2) hipLaunchKernelGGL(loss_bwd_kernel<DUDF_LOSS_S2>, dim3(grid), dim3(256), 0, st, a);
    else return DUDF_E_BADMODE;
    return (int)hipGetLastError();
}

int dudf_launch_s2_stats(const DudfLayout& lo, const float* sdf, float* ws, double* stats, hipStream_t st) {
    hipError_t e = hipMemsetAsync(stats, 0, 3 * sizeof(double), st);
    if (e != hipSuccess) return (int)e;
    const double w0[4] = {0, 0, 0, 0};
    LossArgs a = make_loss_args(lo, nullptr, sdf, 1, w0, 0.0, ws);
    hipLaunchKernelGGL(s2_stats_kernel, dim3(dudf_deterministic() ? 1 : dudf_grid_for(lo.n, 256, kGridCap)), dim3(256), 0, st, a,
                       stats);
    return (int)hipGetLastError();
}

int dudf_launch_s2_terms(const double* stats, const double* w, float* out_terms, hipStream_t st) {
    hipLaunchKernelGGL(s2_terms_kernel, dim3(1), dim3(64), 0, st, stats, w[0], w[1], out_terms);
    return (int)hipGetLastError();
}

int dudf_launch_adam(float* theta, const float* g, float* m, float* v, int64_t n, double lr, double b1, double b2,
                     double eps, int64_t step, double gscale, hipStream_t st) {
    DudfProfScope prof(PROF_ADAM, st);
    float step_size, bc2_sqrt;
    dudf_adam_factors(lr, b1, b2, step, &step_size, &bc2_sqrt);
    hipLaunchKernelGGL(adam_kernel, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), 0, st, theta, g, m, v, n, (float)(1.0 - b1),
                       (float)b2, (float)(1.0 - b2), (float)eps, step_size, bc2_sqrt, (float)gscale);
    return (int)hipGetLastError();
}

void dudf_adam_factors(double lr, double b1, double b2, int64_t step, float* step_size, float* bc2_sqrt) {
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    *step_size = (float)(lr / bc1); *bc2_sqrt = (float)sqrt(bc2);
}

int dudf_launch_adam_sched(float* theta, const float* g, float* m, float* v, int64_t n, double b1, double b2, double eps,
                           const float* sched, int64_t n_rows, const int64_t* row, double gscale, hipStream_t st) {
    DudfProfScope prof(PROF_ADAM, st);
    hipLaunchKernelGGL(adam_sched_kernel, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), 0, st, theta, g, m, v, n,
                       (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, sched, n_rows, row, (float)gscale);
    return (int)hipGetLastError();
}

int dudf_launch_read_stash(const DudfLayout& lo, const float* src, int layer, int channel, float* out, hipStream_t st, int per_quad, int p24,
                           const float* fx) {
    hipLaunchKernelGGL(read_stash_kernel, dim3(dudf_grid_for(lo.n * lo.H, 256, kGridCap)), dim3(256), 0, st,
                       src + (int64_t)layer * (p24 ? lo.stash_layer / 4 * 3 : lo.stash_layer), out, lo.n, lo.n_h, lo.ncol_h, lo.np,
                       lo.H, channel, per_quad, p24, fx ? fx + (int64_t)layer * lo.np : nullptr);
    return (int)hipGetLastError();
}

int dudf_launch_copy_in(const DudfLayout& lo, const float* ybar, const float* gbar, float* ws, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(copy_in_kernel, dim3(dudf_grid_for(lo.np, 256, kGridCap)), dim3(256), 0, st, ybar, gbar, ws + lo.ws_ybar,
                       ws + lo.ws_gbar, lo.n, lo.n_h, lo.ncol_h, lo.np);
    return (int)hipGetLastError();
}

int dudf_launch_make_x4(const DudfLayout& lo, const float* x, float* ws, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    hipLaunchKernelGGL(make_x4_kernel, dim3(dudf_grid_for(lo.np, 256, kGridCap)), dim3(256), 0, st, x, ws + lo.ws_x4, lo.n, lo.n_h,
                       lo.ncol_h, lo.np);
    return (int)hipGetLastError();
}
