// The training step behind the C ABI: sweep sequencing (dudf_context.h), the loss / weight-gradient / Adam entry points, workspace
// sizes and the debug reads.  See include/dudf_hip.h.
#include "dudf_context.h"

namespace {

int split_mask() { return dudf_split_mask(dudf_options()); }

int check_ws(const DudfLayout& lo, const void* ws, size_t bytes) {
    if (int rc = dudf_check_buffer(ws, bytes, lo.total_bytes)) return rc;
    if (lo.np > (1ll << 25)) return DUDF_E_BADCFG;          // 32-bit lane BYTE offsets inside a stash layer (4 np granules of 16 B)
    return 0;
}

SweepRequest make_request(int which, int H, const SweepArgs& a) {
    return SweepRequest{which, H, a.L, a.store_s, a.store_c, a.train, a.have_e, a.split, a.p24, a.ebound != nullptr, a.zbound != nullptr};
}

// what the loss entry points accept: the forward loss_s1 and loss_siren, the backward loss_s2 as well (with its statistics);
// Hessian-path points only under loss_s1 with a Hessian weight
int check_loss_mode(int mode, bool backward, int64_t n_hess, const double* weights, const double* stats) {
    if (mode != DUDF_LOSS_S1 && mode != DUDF_LOSS_SIREN && !(backward && mode == DUDF_LOSS_S2)) return DUDF_E_BADMODE;
    if (mode == DUDF_LOSS_S2 && !stats) return DUDF_E_BADMODE;
    if (n_hess != 0 && !(mode == DUDF_LOSS_S1 && weights[2] != 0.0)) return DUDF_E_BADMODE;
    return 0;
}

// workspace offset (floats) of stash array `which`: 0 S, 1 C, 2 Q, 3 E, 4 A, 5 Z, 6 R, 7 ZS
int64_t stash_offset(const DudfLayout& lo, int which) {
    const int64_t offs[8] = {lo.ws_S, lo.ws_C, lo.ws_Q, lo.ws_E, lo.ws_A, lo.ws_Z, lo.ws_R, lo.ws_ZS};
    return offs[which];
}

}  // namespace

SweepArgs dudf_make_sweep_args(const DudfLayout& lo, const float* theta, float* ws) {
    SweepArgs a;
    a.theta = theta; a.w1b = ws + lo.ws_w1b; a.b1s = ws + lo.ws_b1s; a.w1t16 = ws + lo.ws_w1t16; a.wt = ws + lo.ws_wt;
    a.wimg_f = reinterpret_cast<const char*>(ws + lo.ws_wimg);
    a.wimg_t = a.wimg_f + (size_t)(lo.L - 1) * lo.H * lo.H * 6;
    a.wimg16_f = reinterpret_cast<const char*>(ws + lo.ws_wimg16);
    a.wimg16_t = a.wimg16_f + (size_t)(lo.L - 1) * lo.H * lo.H * 4;
    a.wsc = ws + lo.ws_wsc;
    a.amax = reinterpret_cast<unsigned*>(ws + lo.ws_amax);
    a.ebound = (lo.ws_ebound != lo.ws_amax) ? ws + lo.ws_ebound : nullptr;
    a.zbound = (lo.ws_zbound != lo.ws_amax) ? ws + lo.ws_zbound : nullptr;
    a.nch = lo.ncol_h;
    a.split = split_mask();
    a.clk = nullptr;
    a.x4 = ws + lo.ws_x4; a.y = ws + lo.ws_y; a.g = ws + lo.ws_g; a.ybar = ws + lo.ws_ybar; a.gbar = ws + lo.ws_gbar;
    a.S = ws + lo.ws_S; a.C = ws + lo.ws_C; a.ZS = ws + lo.ws_ZS; a.Q = ws + lo.ws_Q; a.R = ws + lo.ws_R;
    a.E = ws + lo.ws_E; a.A = ws + lo.ws_A; a.Z = ws + lo.ws_Z;
    a.np = lo.np; a.stash_layer = lo.stash_layer;
    a.off_hid = lo.off_hid; a.hid_stride = lo.hid_stride; a.off_wo = lo.off_wo; a.off_bo = lo.off_bo;
    a.L = lo.L; a.w0 = lo.w0;
    a.store_s = 0; a.store_c = 0; a.train = 0; a.have_e = 1;
    a.tile0 = 0; a.ntiles = 0; a.hess = 0;
    a.p24 = lo.p24;
    a.fxs = nullptr;
    return a;
}

int dudf_launch_range(int which, int H, SweepArgs a, hipStream_t st) {
    const SweepChoice c = dudf_choose_sweep(make_request(which, H, a), dudf_options());
    if (c.status) return c.status;
    DudfProfScope prof(PROF_SWEEP_FWD + (which & 3), st);
    if (which <= SWEEP_ADJ_REV) dudf_note_products(PROF_SWEEP_FWD + which, c.products);
    a.store_s = c.store_s; a.store_c = c.store_c;
    if (c.family == DUDF_FAM_F32) return dudf_launch_sweep(c, a, st);
    if (which <= SWEEP_ADJ_REV) a.clk = dudf_prof_clk(PROF_SWEEP_FWD + which);       // plain columns only
    return dudf_launch_sweep_bf16(c, a, st);
}

int dudf_run_sweep(int base, const DudfLayout& lo, SweepArgs a, hipStream_t st) {
    int rc = 0;
    if ((lo.p24 & 1) && base >= SWEEP_FWD && base <= SWEEP_ADJ_REV) a.fxs = a.S - lo.ws_S + lo.ws_fx[base];   // (a.S - lo.ws_S = the workspace base)
    SweepArgs aq = a, ap = a;
    aq.tile0 = 0; aq.ntiles = (int)(lo.ncol_h / DUDF_TILE_PTS); aq.hess = 1;
    ap.tile0 = aq.ntiles; ap.ntiles = (int)(lo.ncol_n / DUDF_TILE_PTS); ap.hess = 0;
    if (lo.ncol_h > 0 && lo.ncol_n > 0) {
        const SweepChoice c = dudf_choose_pair(make_request(base, lo.H, a), dudf_options());
        if (c.status == 0) {
            DudfProfScope prof(PROF_SWEEP_FWD + base, st);
            dudf_note_products(PROF_SWEEP_FWD + base, c.products);
            ap.clk = dudf_prof_clk(PROF_SWEEP_FWD + base);
            return dudf_launch_sweep_pair(c, aq, ap, st);
        }
    }
    if (lo.ncol_h > 0 && (rc = dudf_launch_range(base + 4, lo.H, aq, st))) return rc;
    if (lo.ncol_n > 0 && (rc = dudf_launch_range(base, lo.H, ap, st))) return rc;
    return 0;
}

int dudf_open_ctx(const dudf_net_cfg* cfg, int64_t n, int64_t n_h, void* workspace, size_t bytes, void* stream, DudfCtx* c,
                  int query_only) {
    int rc = dudf_make_layout(cfg, n, n_h, &c->lo, query_only);
    if (rc) return rc;
    if ((rc = check_ws(c->lo, workspace, bytes))) return rc;
    c->st = reinterpret_cast<hipStream_t>(stream);
    c->ws = reinterpret_cast<float*>(workspace);
    return 0;
}

int dudf_forward_common(DudfCtx& c, const float* theta, const float* x, int train, bool reverse) {
    int rc;
    // One launch: A-operand forms of theta, x4, zeros for the loss sums / ticket and the running maxima.  The bf16x3 images
    // and W^T are packed only when a kernel that reads them can run: everything except a training step of plain columns
    // whose four sweeps are all fp16x3 (Hessian quads, jets, A/B modes, very deep nets: bf16x6; f32-input kernels: W^T).
    const DudfLayout& lo = c.lo;
    const bool all16 = train && lo.ncol_h == 0 && dudf_use_bf16_sweeps() && (split_mask() & 15) == 15 && lo.L <= 32;
    const int need = (all16 ? 0 : 1) | (!dudf_use_bf16_sweeps() ? 2 : 0);
    rc = (lo.L >= 2) ? dudf_launch_prep(lo, theta, x, c.ws, need, c.st) : DUDF_E_UNSUPPORTED;
    if (rc == DUDF_E_UNSUPPORTED) {                     // widths without 16-bit weight images: the separate kernels
        if ((rc = dudf_launch_pack(c.lo, theta, c.ws, c.st))) return rc;
        if (dudf_use_bf16_sweeps() && (rc = dudf_launch_pack_bf16(c.lo, theta, c.ws, c.st))) return rc;
        if (x && (rc = dudf_launch_make_x4(c.lo, x, c.ws, c.st))) return rc;
        hipError_t e = hipMemsetAsync(c.ws + c.lo.ws_acc, 0, (size_t)2 * DUDF_NACC * sizeof(float), c.st);
        if (e == hipSuccess) e = hipMemsetAsync(c.ws + c.lo.ws_amax, 0, (size_t)4 * c.lo.L * sizeof(unsigned), c.st);
        if (e != hipSuccess) return (int)e;
    } else if (rc) {
        return rc;
    }
    SweepArgs a = dudf_make_sweep_args(c.lo, theta, c.ws);
    // what the forward sweep has to leave behind: h_l only for training (weight gradients, r_l), cos if any later sweep
    // runs — a value-only query stores nothing, a value+gradient query half of what training does
    a.store_s = train ? 1 : 0; a.store_c = (reverse || train) ? 1 : 0; a.train = train;
    if ((rc = dudf_run_sweep(SWEEP_FWD, c.lo, a, c.st))) return rc;
    if (reverse && (rc = dudf_run_sweep(SWEEP_REV, c.lo, a, c.st))) return rc;
    return 0;
}

int dudf_backward_common(DudfCtx& c, const float* theta, int have_g, float* dtheta, int accumulate, bool zeroed) {
    int rc;
    if (!accumulate && !zeroed) {
        hipError_t e = hipMemsetAsync(dtheta, 0, (size_t)c.lo.n_theta * sizeof(float), c.st);
        if (e != hipSuccess) return (int)e;
    }
    if ((rc = dudf_backward_sweeps(c, theta, have_g, zeroed))) return rc;
    return dudf_launch_wgrad(c.lo, c.ws, dtheta, have_g, c.st);
}

int dudf_backward_sweeps(DudfCtx& c, const float* theta, int have_g, bool zeroed) {
    int rc;
    SweepArgs a = dudf_make_sweep_args(c.lo, theta, c.ws);
    a.train = 1;
    if (dudf_split_fp16() && !(zeroed && 2 * c.lo.L <= 256)) {   // a backward may run several times per forward: A_l and zbar_l start over
        hipError_t e = hipMemsetAsync(c.ws + c.lo.ws_amax + c.lo.L, 0, (size_t)2 * c.lo.L * sizeof(unsigned), c.st);
        if (e != hipSuccess) return (int)e;
    }
    if (have_g) {
        if ((rc = dudf_run_sweep(SWEEP_ADJ_FWD, c.lo, a, c.st))) return rc;
    } else {
        a.have_e = 0;                                   // no df/dx terms: e_l == 0 in the reverse adjoint sweep
    }
    return dudf_run_sweep(SWEEP_ADJ_REV, c.lo, a, c.st);
}

extern "C" {

int dudf_sweeps_bf16x6(const dudf_net_cfg* cfg) {
    if (!cfg) return 0;
    const SweepRequest r = {SWEEP_FWD, cfg->hidden, cfg->n_hidden_layers, 0, 0, 0, 1, split_mask(), 0, false, false};   // a value query
    const SweepChoice c = dudf_choose_sweep(r, dudf_options());
    return (c.status == 0 && c.family != DUDF_FAM_F32) ? 1 : 0;
}

int64_t dudf_theta_count(const dudf_net_cfg* cfg) {
    DudfLayout lo;
    if (dudf_make_layout(cfg, 1, 0, &lo)) return -1;
    return lo.n_theta;
}

size_t dudf_workspace_bytes(const dudf_net_cfg* cfg, int64_t n) { return dudf_workspace_bytes_hess(cfg, n, 0); }

size_t dudf_workspace_bytes_query(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess) {
    DudfLayout lo;
    if (dudf_make_layout(cfg, n, n_hess, &lo, 1)) return 0;
    return lo.total_bytes;
}

size_t dudf_workspace_bytes_hess(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess) {
    DudfLayout lo;
    if (dudf_make_layout(cfg, n, n_hess, &lo)) return 0;
    return lo.total_bytes;
}

int dudf_stash_mode(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess) {
    DudfLayout lo;
    if (dudf_make_layout(cfg, n, n_hess, &lo)) return -1;
    return lo.p24;
}

int dudf_loss_forward(const dudf_net_cfg* cfg, int mode, const float* theta, const float* x, const float* normals,
                      const float* sdf, int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights,
                      double alpha, float* out_terms, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_loss_mode(mode, false, n_hess, weights, nullptr);
    if (rc) return rc;
    DudfCtx c;
    if ((rc = dudf_open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c))) return rc;
    if ((rc = dudf_forward_common(c, theta, x, 1, true))) return rc;
    return dudf_launch_loss_fwd(c.lo, mode, normals, sdf, n_global, weights, alpha, c.ws, out_terms, c.st);
}

int dudf_s2_forward_stats(const dudf_net_cfg* cfg, const float* theta, const float* x, const float* sdf,
                          int64_t n_local, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n_local, 0, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if ((rc = dudf_forward_common(c, theta, x, 1, false))) return rc;
    return dudf_launch_s2_stats(c.lo, sdf, c.ws, stats, c.st);
}

int dudf_s2_terms(const double* stats, const double* weights, float* out_terms, void* stream) {
    return dudf_launch_s2_terms(stats, weights, out_terms, reinterpret_cast<hipStream_t>(stream));
}

int dudf_loss_backward(const dudf_net_cfg* cfg, int mode, const float* theta, const float* x, const float* normals,
                       const float* sdf, int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights,
                       double alpha, const float* cot, const double* stats, float* dtheta, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_loss_mode(mode, true, n_hess, weights, stats);
    if (rc) return rc;
    DudfCtx c;
    if ((rc = dudf_open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c))) return rc;
    (void)x;
    if ((rc = dudf_launch_loss_bwd(c.lo, mode, normals, sdf, n_global, weights, alpha, cot, stats, c.ws, c.st,
                                   accumulate ? nullptr : dtheta, c.lo.n_theta)))
        return rc;
    return dudf_backward_common(c, theta, mode != DUDF_LOSS_S2, dtheta, accumulate, true);
}

int dudf_loss_backward_sweeps(const dudf_net_cfg* cfg, int mode, const float* theta, const float* normals, const float* sdf,
                              int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights, double alpha,
                              const float* cot, const double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_loss_mode(mode, true, n_hess, weights, stats);
    if (rc) return rc;
    DudfCtx c;
    if ((rc = dudf_open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c))) return rc;
    if ((rc = dudf_launch_loss_bwd(c.lo, mode, normals, sdf, n_global, weights, alpha, cot, stats, c.ws, c.st))) return rc;
    return dudf_backward_sweeps(c, theta, mode != DUDF_LOSS_S2, true);
}

int dudf_weight_gradient(const dudf_net_cfg* cfg, int64_t n_local, int64_t n_hess, int have_gradient_terms, int layer_begin,
                         int layer_end, float* dtheta, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    const DudfLayout& lo = c.lo;
    if (layer_begin == -1) {                            // the two thin layers (0 and L) together: one pass of their kernel
        if (!accumulate) {
            hipError_t e = hipMemsetAsync(dtheta, 0, (size_t)lo.off_hid * sizeof(float), c.st);
            if (e == hipSuccess) e = hipMemsetAsync(dtheta + lo.off_wo, 0, (size_t)(lo.n_theta - lo.off_wo) * sizeof(float), c.st);
            if (e != hipSuccess) return (int)e;
        }
        return dudf_launch_wgrad(lo, c.ws, dtheta, have_gradient_terms, c.st, 0, 1);
    }
    if (layer_begin < 0 || layer_end > lo.L + 1 || layer_begin >= layer_end) return DUDF_E_BADCFG;
    if (!accumulate) {                                  // zero exactly the slices this call owns
        auto zero = [&](int64_t off, int64_t cnt) { return hipMemsetAsync(dtheta + off, 0, (size_t)cnt * sizeof(float), c.st); };
        hipError_t e = hipSuccess;
        if (layer_begin <= 0) e = zero(0, lo.off_hid);
        const int hb = layer_begin < 1 ? 1 : layer_begin, he = layer_end > lo.L ? lo.L : layer_end;
        if (e == hipSuccess && he > hb) e = zero(lo.off_hid + (int64_t)(hb - 1) * lo.hid_stride, (int64_t)(he - hb) * lo.hid_stride);
        if (e == hipSuccess && layer_end >= lo.L + 1) e = zero(lo.off_wo, lo.n_theta - lo.off_wo);
        if (e != hipSuccess) return (int)e;
    }
    return dudf_launch_wgrad(lo, c.ws, dtheta, have_gradient_terms, c.st, layer_begin, layer_end);
}

int dudf_fields_forward(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f,
                        float* out_g, void* workspace, size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if ((rc = dudf_forward_common(c, theta, x, 1, true))) return rc;
    return dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, nullptr, c.st);
}

int dudf_fields_backward(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, const float* ybar,
                         const float* gbar, float* dtheta, int accumulate, void* workspace, size_t workspace_bytes,
                         void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    (void)x;
    if ((rc = dudf_launch_copy_in(c.lo, ybar, gbar, c.ws, c.st))) return rc;
    return dudf_backward_common(c, theta, gbar != nullptr, dtheta, accumulate);
}

int dudf_adam_step(float* theta, const float* dtheta, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                   double beta1, double beta2, double eps, int64_t step, double grad_scale, void* stream) {
    if (n <= 0 || step < 1) return DUDF_E_BADCFG;
    return dudf_launch_adam(theta, dtheta, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, grad_scale,
                            reinterpret_cast<hipStream_t>(stream));
}

int dudf_adam_schedule(const double* lr, int64_t n_steps, int64_t first_step, double beta1, double beta2, float* out) {
    if (!lr || !out || n_steps < 0 || first_step < 1) return DUDF_E_BADCFG;
    for (int64_t i = 0; i < n_steps; ++i) dudf_adam_factors(lr[i], beta1, beta2, first_step + i, out + 2 * i, out + 2 * i + 1);
    return 0;
}

int dudf_adam_step_scheduled(float* theta, const float* dtheta, float* exp_avg, float* exp_avg_sq, int64_t n, double beta1,
                             double beta2, double eps, const float* sched, int64_t n_rows, const int64_t* row, double grad_scale,
                             void* stream) {
    if (n <= 0 || !sched || !row || n_rows < 1) return DUDF_E_BADCFG;
    return dudf_launch_adam_sched(theta, dtheta, exp_avg, exp_avg_sq, n, beta1, beta2, eps, sched, n_rows, row, grad_scale,
                                  reinterpret_cast<hipStream_t>(stream));
}

int dudf_debug_read_stash(const dudf_net_cfg* cfg, int which, int layer, int channel, int64_t n, int64_t n_hess,
                          float* out, void* workspace, size_t workspace_bytes, void* stream) {
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, n_hess, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if (layer < 0 || layer >= c.lo.L || channel < 0 || channel > 3) return DUDF_E_BADCFG;
    const DudfLayout& lo = c.lo;
    if (which < 0 || which > 7) return DUDF_E_BADMODE;
    // E, R (bit 1): 24-bit floats, tile-major; C (bit 2): 24-bit fixed point, same granules; S, Q, A, Z (bit 0): fixed point relative to
    // the column scales the sweeps leave in ws_fx
    const bool sqaz = which == 0 || which == 2 || which == 4 || which == 5;
    const int b24 = which == 7 ? 0 : which == 1 ? ((lo.p24 & 4) ? 2 : 0) : sqaz ? ((lo.p24 & 1) ? 3 : 0) : ((lo.p24 & 2) ? 1 : 0);
    const int fxi = which == 0 ? 0 : which == 2 ? 1 : which == 4 ? 2 : 3;
    return dudf_launch_read_stash(lo, c.ws + stash_offset(lo, which), layer, channel, out, c.st, which == 1, b24,
                                  b24 == 3 ? c.ws + lo.ws_fx[fxi] : nullptr);   // C: one copy per quad
}

int dudf_debug_stash_layout(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess, int64_t* out) {
    DudfLayout lo;
    int rc = dudf_make_layout(cfg, n, n_hess, &lo);
    if (rc) return rc;
    if (!out) return DUDF_E_BADCFG;
    for (int i = 0; i < 8; ++i) out[i] = stash_offset(lo, i) * (int64_t)sizeof(float);
    out[8] = lo.np * 16;                                  // bytes between two feature-quad rows
    out[9] = lo.stash_layer * (int64_t)sizeof(float);     // bytes between two layers
    return 0;
}

int dudf_debug_kernel_choice(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess, int which, int flags, char* name, size_t name_len) {
    DudfLayout lo;
    int rc = dudf_make_layout(cfg, n, n_hess, &lo, (flags & 16) != 0);
    if (rc) return rc;
    if (!name || name_len == 0) return DUDF_E_BADCFG;
    name[0] = 0;
    SweepChoice c;
    if (which == DUDF_CHOICE_WGRAD) {
        c = dudf_choose_wgrad(WgradRequest{lo.H, lo.L, lo.p24 & 1, lo.np}, dudf_options());
    } else {
        const SweepRequest r = {which & 15, lo.H, lo.L, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, (flags >> 3) & 1, split_mask(), lo.p24,
                                lo.ws_ebound != lo.ws_amax, lo.ws_zbound != lo.ws_amax};
        c = (which & DUDF_CHOICE_PAIR) ? dudf_choose_pair(r, dudf_options()) : dudf_choose_sweep(r, dudf_options());
    }
    if (c.status == 0 && dudf_choice_name(c, name, name_len) >= (int)name_len) return DUDF_E_WORKSPACE;
    return c.status;
}

}  // extern "C"
