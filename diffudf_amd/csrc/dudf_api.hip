// C-ABI glue: argument checks, workspace layout, kernel sequencing.  See include/dudf_hip.h.
#include "dudf_internal.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// ---- per-kernel HIP-event timing ---------------------------------------------------------------------------
namespace {
struct ProfRec { int slot; hipEvent_t e0, e1; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t g_prof_open[PROF_NSLOTS];
const char* kProfNames[PROF_NSLOTS] = {"pack", "sweep_fwd", "sweep_rev", "sweep_adj_fwd", "sweep_adj_rev",
                                       "wgrad_hidden", "wgrad_small", "loss_fwd", "loss_bwd", "adam", "other"};
unsigned long long* g_prof_clk = nullptr;               // device: [PROF_NSLOTS][2]
hipEvent_t prof_event() {
    if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
}  // namespace

namespace { int g_products[PROF_NSLOTS] = {0}; }
void dudf_note_products(int slot, int products) { if (slot >= 0 && slot < PROF_NSLOTS) g_products[slot] = products; }

unsigned long long* dudf_prof_clk(int slot) { return (g_prof_on && g_prof_clk) ? g_prof_clk + 2 * slot : nullptr; }

void dudf_prof_begin(int slot, hipStream_t st) {
    if (!g_prof_on) return;
    g_prof_open[slot] = prof_event();
    (void)hipEventRecord(g_prof_open[slot], st);
}
void dudf_prof_end(int slot, hipStream_t st) {
    if (!g_prof_on) return;
    hipEvent_t e1 = prof_event();
    (void)hipEventRecord(e1, st);
    g_prof_recs.push_back({slot, g_prof_open[slot], e1});
}

// ---- run-time options (dudf_set_option / dudf_get_option in the C ABI; rounds 1-4 read environment variables once, at the first
// call — VERDICT r04 #8).  Process-wide, plain ints, read at every call: a mode switches in-process, between two steps.
#ifndef DUDF_WGRAD_BUFFERS_DEFAULT
#define DUDF_WGRAD_BUFFERS_DEFAULT 4
#endif
namespace {
struct OptDesc { const char* name; int lo, hi, def; };
enum { OPT_DETERMINISTIC = 0, OPT_SPLIT, OPT_SPLIT_QUADS, OPT_SWEEP_FAMILY, OPT_STASH, OPT_WGRAD_FAMILY, OPT_WGRAD_TR, OPT_PAIR_LAUNCH,
       OPT_WGRAD_MAXWG, OPT_WGRAD_BUFFERS, OPT_COUNT };
const OptDesc kOpts[OPT_COUNT] = {
    {"deterministic", 0, 1, 0},            // 1: every cross-workgroup sum of the training path has ONE owner (bit-reproducible; slow)
    {"split", 0, 1, 1},                    // operand split of the 16-bit matrix cores: 1 = fp16 hi/lo, three products; 0 = bf16x3, six
    {"split_quads", 0, 1, 1},              // the Hessian quads / jets on fp16x3 as well (0: bf16x6)
    {"sweep_family", 0, 1, 1},             // 1 = the 16-bit-core sweeps where built; 0 = the f32-input MFMA kernel everywhere (A/B reference)
    {"stash", 0, 15, DUDF_STASH_DEFAULT},  // REQUESTED stash mask (dudf_stash_mode reports what a workspace gets)
    {"wgrad_family", 0, 2, 0},             // weight-gradient GEMM: 0 = cooperative split (default), 1 = f32-input MFMA, 2 = bf16x6 per-wave split
    {"wgrad_tr", 0, 1, 0},                 // fp32 rows staged through the [column][feature] image + transposed fragment reads
    {"pair_launch", 0, 1, 1},              // quads + plain columns of a training sweep in ONE grid
    {"wgrad_max_workgroups", 8, 256, 256}, // cap of the weight-gradient GEMM's grid (a multi-GPU step leaves CUs to RCCL)
    {"wgrad_buffers", 3, 4, DUDF_WGRAD_BUFFERS_DEFAULT},   // LDS image buffers of the 24-bit-operand weight-gradient GEMM (4: one poll per stage instead of two)
};
int g_opt[OPT_COUNT] = {0, 1, 1, 1, DUDF_STASH_DEFAULT, 0, 0, 1, 256, DUDF_WGRAD_BUFFERS_DEFAULT};
}  // namespace

int dudf_wgrad_max_workgroups() { return g_opt[OPT_WGRAD_MAXWG]; }
bool dudf_deterministic() { return g_opt[OPT_DETERMINISTIC] != 0; }
bool dudf_split_fp16() { return g_opt[OPT_SPLIT] != 0; }
DudfOptions dudf_options() {
    DudfOptions o;
    o.deterministic = g_opt[OPT_DETERMINISTIC]; o.split = g_opt[OPT_SPLIT]; o.split_quads = g_opt[OPT_SPLIT_QUADS];
    o.sweep_family = g_opt[OPT_SWEEP_FAMILY]; o.stash = g_opt[OPT_STASH]; o.wgrad_family = g_opt[OPT_WGRAD_FAMILY];
    o.wgrad_tr = g_opt[OPT_WGRAD_TR]; o.pair_launch = g_opt[OPT_PAIR_LAUNCH]; o.wgrad_max_workgroups = g_opt[OPT_WGRAD_MAXWG];
    o.wgrad_buffers = g_opt[OPT_WGRAD_BUFFERS];
    return o;
}

namespace {
// option sweep_family = 0 keeps every sweep on the f32-input MFMA kernel (A/B testing); default: the 16-bit cores where built
bool use_bf16_sweeps() { return g_opt[OPT_SWEEP_FAMILY] != 0; }
int split_mask() { return dudf_split_mask(dudf_options()); }
}  // namespace

namespace {

int check_ws(const DudfLayout& lo, const void* ws, size_t bytes) {
    if (!ws || bytes < lo.total_bytes || (reinterpret_cast<uintptr_t>(ws) & 255)) return DUDF_E_WORKSPACE;
    if (lo.np > (1ll << 25)) return DUDF_E_BADCFG;          // 32-bit lane BYTE offsets inside a stash layer (4 np granules of 16 B)
    return 0;
}

SweepArgs make_sweep_args(const DudfLayout& lo, const float* theta, float* ws) {
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

SweepRequest make_request(int which, int H, const SweepArgs& a) {
    return SweepRequest{which, H, a.L, a.store_s, a.store_c, a.train, a.have_e, a.split, a.p24, a.ebound != nullptr, a.zbound != nullptr};
}

// one column range of a sweep: build the request, choose, note the products, launch
int launch_range(int which, int H, SweepArgs a, hipStream_t st) {
    const SweepChoice c = dudf_choose_sweep(make_request(which, H, a), dudf_options());
    if (c.status) return c.status;
    DudfProfScope prof(PROF_SWEEP_FWD + (which & 3), st);
    if (which <= SWEEP_ADJ_REV) dudf_note_products(PROF_SWEEP_FWD + which, c.products);
    a.store_s = c.store_s; a.store_c = c.store_c;
    if (c.family == DUDF_FAM_F32) return dudf_launch_sweep(c, a, st);
    if (which <= SWEEP_ADJ_REV) a.clk = dudf_prof_clk(PROF_SWEEP_FWD + which);       // plain columns only
    return dudf_launch_sweep_bf16(c, a, st);
}

// one sweep over both column ranges: Hessian quads and plain columns in one grid where a pair kernel is built (a training batch
// with Hessian-path points), otherwise the quads first, then the plain columns
int run_sweep(int base, const DudfLayout& lo, SweepArgs a, hipStream_t st) {
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
    if (lo.ncol_h > 0 && (rc = launch_range(base + 4, lo.H, aq, st))) return rc;
    if (lo.ncol_n > 0 && (rc = launch_range(base, lo.H, ap, st))) return rc;
    return 0;
}

struct Ctx {
    DudfLayout lo;
    hipStream_t st;
    float* ws;
};

int open_ctx(const dudf_net_cfg* cfg, int64_t n, int64_t n_h, void* workspace, size_t bytes, void* stream, Ctx* c,
             int query_only = 0) {
    int rc = dudf_make_layout(cfg, n, n_h, &c->lo, query_only);
    if (rc) return rc;
    if ((rc = check_ws(c->lo, workspace, bytes))) return rc;
    c->st = reinterpret_cast<hipStream_t>(stream);
    c->ws = reinterpret_cast<float*>(workspace);
    return 0;
}

// pack + x4 + forward (+ reverse) sweeps with the given stash flags.  x == nullptr: x4 was already filled (grid query).
// `train` = keep what the adjoint sweeps need; the forward sweep always runs its stash-everything variant (the only
// one the register allocator handles without spills), queries merely skip the reverse sweep's stores.
int forward_common(Ctx& c, const float* theta, const float* x, int train, bool reverse) {
    int rc;
    // One launch: A-operand forms of theta, x4, zeros for the loss sums / ticket and the running maxima.  The bf16x3 images
    // and W^T are packed only when a kernel that reads them can run: everything except a training step of plain columns
    // whose four sweeps are all fp16x3 (Hessian quads, jets, A/B modes, very deep nets: bf16x6; f32-input kernels: W^T).
    const DudfLayout& lo = c.lo;
    const bool all16 = train && lo.ncol_h == 0 && use_bf16_sweeps() && (split_mask() & 15) == 15 && lo.L <= 32;
    const int need = (all16 ? 0 : 1) | (!use_bf16_sweeps() ? 2 : 0);
    rc = (lo.L >= 2) ? dudf_launch_prep(lo, theta, x, c.ws, need, c.st) : DUDF_E_UNSUPPORTED;
    if (rc == DUDF_E_UNSUPPORTED) {                     // widths without 16-bit weight images: the separate kernels
        if ((rc = dudf_launch_pack(c.lo, theta, c.ws, c.st))) return rc;
        if (use_bf16_sweeps() && (rc = dudf_launch_pack_bf16(c.lo, theta, c.ws, c.st))) return rc;
        if (x && (rc = dudf_launch_make_x4(c.lo, x, c.ws, c.st))) return rc;
        hipError_t e = hipMemsetAsync(c.ws + c.lo.ws_acc, 0, (size_t)2 * DUDF_NACC * sizeof(float), c.st);
        if (e == hipSuccess) e = hipMemsetAsync(c.ws + c.lo.ws_amax, 0, (size_t)4 * c.lo.L * sizeof(unsigned), c.st);
        if (e != hipSuccess) return (int)e;
    } else if (rc) {
        return rc;
    }
    SweepArgs a = make_sweep_args(c.lo, theta, c.ws);
    // what the forward sweep has to leave behind: h_l only for training (weight gradients, r_l), cos if any later sweep
    // runs — a value-only query stores nothing, a value+gradient query half of what training does
    a.store_s = train ? 1 : 0; a.store_c = (reverse || train) ? 1 : 0; a.train = train;
    if ((rc = run_sweep(SWEEP_FWD, c.lo, a, c.st))) return rc;
    if (reverse && (rc = run_sweep(SWEEP_REV, c.lo, a, c.st))) return rc;
    return 0;
}

// the adjoint sweeps; the weight gradients follow (all layers at once, or layer ranges through dudf_weight_gradient)
int backward_sweeps(Ctx& c, const float* theta, int have_g, bool zeroed = false);

// `zeroed`: the caller's cotangent kernel (loss_bwd) already cleared d(theta) and the running maxima on its way
int backward_common(Ctx& c, const float* theta, int have_g, float* dtheta, int accumulate, bool zeroed = false) {
    int rc;
    if (!accumulate && !zeroed) {
        hipError_t e = hipMemsetAsync(dtheta, 0, (size_t)c.lo.n_theta * sizeof(float), c.st);
        if (e != hipSuccess) return (int)e;
    }
    if ((rc = backward_sweeps(c, theta, have_g, zeroed))) return rc;
    return dudf_launch_wgrad(c.lo, c.ws, dtheta, have_g, c.st);
}

int backward_sweeps(Ctx& c, const float* theta, int have_g, bool zeroed) {
    int rc;
    SweepArgs a = make_sweep_args(c.lo, theta, c.ws);
    a.train = 1;
    if (dudf_split_fp16() && !(zeroed && 2 * c.lo.L <= 256)) {   // a backward may run several times per forward: A_l and zbar_l start over
        hipError_t e = hipMemsetAsync(c.ws + c.lo.ws_amax + c.lo.L, 0, (size_t)2 * c.lo.L * sizeof(unsigned), c.st);
        if (e != hipSuccess) return (int)e;
    }
    if (have_g) {
        if ((rc = run_sweep(SWEEP_ADJ_FWD, c.lo, a, c.st))) return rc;
    } else {
        a.have_e = 0;                                   // no df/dx terms: e_l == 0 in the reverse adjoint sweep
    }
    return run_sweep(SWEEP_ADJ_REV, c.lo, a, c.st);
}

}  // namespace

extern "C" {

const char* dudf_version(void) {
    return "dudf_hip 0.8 (gfx950: fp16x3 / bf16x6 MFMA sweeps and weight-gradient GEMM at fp32 accuracy, f32-input MFMA variants, "
           "Hessian quads, third-order jets, GPU sampler, ray marching, point-cloud extraction)";
}

int dudf_split_mode(void) {
    return split_mask() | (dudf_split_fp16() ? 16 : 0);
}

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

size_t dudf_workspace_bytes(const dudf_net_cfg* cfg, int64_t n) {
    DudfLayout lo;
    if (dudf_make_layout(cfg, n, 0, &lo)) return 0;
    return lo.total_bytes;
}

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

int dudf_query(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f, float* out_g,
               void* workspace, size_t workspace_bytes, void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = forward_common(c, theta, x, 0, out_g != nullptr))) return rc;
    return dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, nullptr, c.st);
}

int dudf_query_hessian(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f,
                       float* out_g, float* out_h, void* workspace, size_t workspace_bytes, void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n, n, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = forward_common(c, theta, x, 0, true))) return rc;
    return dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, out_h, c.st);
}

int dudf_query_frame(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, float* out_f,
                     float* out_g, float* out_h, float* out_lambda, float* out_v, void* workspace,
                     size_t workspace_bytes, void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n, n, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = forward_common(c, theta, x, 0, true))) return rc;
    if ((rc = dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, out_h, c.st))) return rc;
    return dudf_launch_field_features(c.lo, c.ws, 0, 1.0, nullptr, nullptr, nullptr, out_lambda, out_v, c.st);
}

}  // extern "C"

namespace {
// curvature query workspace = [Hessian-query layout of n points][lam 3n][V 9n][jet x4 4*npj][jet y npj]
struct CurvLayout { DudfLayout q; int64_t npj, o_lam, o_V, o_x4, o_y, o_relay; size_t total_bytes; };
int make_curv_layout(const dudf_net_cfg* cfg, int64_t n, CurvLayout* cl) {
    int rc = dudf_make_layout(cfg, n, n, &cl->q, 1);
    if (rc) return rc;
    cl->npj = (16 * n + DUDF_TILE_PTS - 1) / DUDF_TILE_PTS * DUDF_TILE_PTS;
    if (cl->npj == 0) cl->npj = DUDF_TILE_PTS;
    if (cl->npj > (1ll << 25)) return DUDF_E_BADCFG;
    int64_t o = (int64_t)(cl->q.total_bytes / sizeof(float));
    auto take = [&](int64_t cnt) { int64_t r = o; o += (cnt + 63) / 64 * 64; return r; };
    cl->o_lam = take(3 * n); cl->o_V = take(9 * n); cl->o_x4 = take(4 * cl->npj); cl->o_y = take(cl->npj);
    // 512-wide layers: a layer's outputs reach the next one through memory (dudf_sweep_wide.hip, sweep_tile_w) — one layer's
    // worth of the jet columns, reused by every layer
    cl->o_relay = cl->q.H == 512 ? take((int64_t)cl->q.H * cl->npj) : cl->o_y;
    cl->total_bytes = (size_t)o * sizeof(float);
    return 0;
}
}  // namespace

extern "C" {

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
    if (!workspace || workspace_bytes < cl.total_bytes || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return DUDF_E_WORKSPACE;
    if (n <= 0) return 0;
    Ctx c;
    c.lo = cl.q; c.st = reinterpret_cast<hipStream_t>(stream); c.ws = reinterpret_cast<float*>(workspace);
    if ((rc = check_ws(c.lo, workspace, workspace_bytes))) return rc;
    // 1. value, df/dx, Hessian (forward-over-reverse quads) and the eigen-frame of the Hessian
    if ((rc = forward_common(c, theta, x, 0, true))) return rc;
    float* lam = c.ws + cl.o_lam; float* V = c.ws + cl.o_V;
    if ((rc = dudf_launch_field_features(c.lo, c.ws, 0, 1.0, nullptr, nullptr, nullptr, lam, V, c.st))) return rc;
    // 2. third-order Taylor jet in the three frame directions: one 16-column tile per point
    if ((rc = dudf_launch_make_x4_jet(x, V, n, cl.npj, c.ws + cl.o_x4, c.st))) return rc;
    SweepArgs a = make_sweep_args(c.lo, theta, c.ws);
    a.x4 = c.ws + cl.o_x4; a.y = c.ws + cl.o_y; a.np = cl.npj; a.stash_layer = (int64_t)c.lo.H * cl.npj;
    if (c.lo.H == 512) { a.S = c.ws + cl.o_relay; a.stash_layer = 0; }     // every layer's slot is the same one
    a.tile0 = 0; a.ntiles = (int)(cl.npj / DUDF_TILE_PTS); a.hess = 1;
    if ((rc = launch_range(SWEEP_FWD_J, c.lo.H, a, c.st))) return rc;
    // 3. first-order eigenvector perturbation
    if ((rc = dudf_launch_curvature(c.ws + cl.o_y, lam, V, n, out_mean, out_gauss, out_shape, c.st))) return rc;
    hipError_t e = hipSuccess;
    if (out_lambda) e = hipMemcpyAsync(out_lambda, lam, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c.st);
    if (e == hipSuccess && out_v) e = hipMemcpyAsync(out_v, V, (size_t)n * 9 * sizeof(float), hipMemcpyDeviceToDevice, c.st);
    return (int)e;
}

int dudf_trace_rays(const dudf_net_cfg* cfg, const float* theta, const double* rays, double* t0, unsigned char* mask,
                    unsigned char* hits, int64_t m, int inverse_mode, double alpha, double min_step,
                    double surface_threshold, int max_iterations, int check_every, int* iterations_done,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (inverse_mode < 0 || inverse_mode > 2 || max_iterations < 0 || check_every < 1) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, m, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (iterations_done) *iterations_done = 0;
    if (m <= 0) return 0;
    hipError_t e = hipMemsetAsync(hits, 0, (size_t)m, c.st);
    if (e != hipSuccess) return (int)e;
    if ((rc = dudf_launch_pack(c.lo, theta, c.ws, c.st))) return rc;
    if (use_bf16_sweeps() && (rc = dudf_launch_pack_bf16(c.lo, theta, c.ws, c.st))) return rc;
    SweepArgs a = make_sweep_args(c.lo, theta, c.ws);
    int* active = reinterpret_cast<int*>(c.ws + c.lo.ws_acc);
    int it = 0;
    for (; it < max_iterations; ++it) {
        // value-only queries at the current positions of ALL rays (retired ones are evaluated and ignored: no compaction,
        // no per-iteration host round trip), then the step / hit / retire update of the active ones
        if ((rc = dudf_launch_rays_x4(c.lo, t0, c.ws, c.st))) return rc;
        if ((rc = run_sweep(SWEEP_FWD, c.lo, a, c.st))) return rc;
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
    if (inverse_mode < 0 || inverse_mode > 2 || gd_steps < 0) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, m, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (m <= 0) return 0;
    for (int s = 0; s < gd_steps; ++s) {
        if ((rc = dudf_launch_rays_x4(c.lo, t0, c.ws, c.st))) return rc;
        if ((rc = forward_common(c, theta, nullptr, 0, true))) return rc;
        if ((rc = dudf_launch_rays_descend(c.lo, c.ws, t0, hits, inverse_mode, alpha, min_step, c.st))) return rc;
    }
    return 0;
}

}  // extern "C"

namespace {
// the projection loop of reference src/render_pc.py:43-56 on a context whose x4 already holds the float32 copies of `samples`:
// per step the value+gradient sweeps and ONE kernel (step in double, move, next x4).  The first step packs theta (forward_common);
// the later ones find the A-operand forms where it left them.  counter / quota: round mode (nothing moves once the quota is reached).
int project_steps(Ctx& c, const float* theta, double* samples, int num_steps, int inverse_mode, double alpha, double thresh,
                  double* out_step, double* out_unit, float* out_pre, unsigned char* out_accept, const int64_t* counter,
                  int64_t quota) {
    int rc;
    SweepArgs a = make_sweep_args(c.lo, theta, c.ws);
    a.store_c = 1;
    for (int s = 0; s < num_steps; ++s) {
        if (s == 0) {
            if ((rc = forward_common(c, theta, nullptr, 0, true))) return rc;
        } else {
            if ((rc = run_sweep(SWEEP_FWD, c.lo, a, c.st))) return rc;
            if ((rc = run_sweep(SWEEP_REV, c.lo, a, c.st))) return rc;
        }
        const int last = s + 1 == num_steps;
        if ((rc = dudf_launch_pc_step(c.lo, c.ws, samples, inverse_mode, alpha, thresh, last, out_step, out_unit, out_pre,
                                      out_accept, counter, quota, c.st))) return rc;
    }
    return 0;
}

// round workspace = [value+gradient query layout of n points][samples 3n doubles][proposals 3n doubles][unit gradient 3n doubles][pre-move position 3n]
// [the same, compacted 3n][accept flags n bytes][tile counts + offsets][V 9 chunk][frame-query layout of `chunk` points]
constexpr int64_t kPcFrameChunk = 32768;
struct PcLayout { DudfLayout q; int64_t chunk, o_samples, o_prop, o_unit, o_pre, o_prec, o_accept, o_tiles, o_V, o_frame; size_t frame_bytes, total_bytes; };
int make_pc_layout(const dudf_net_cfg* cfg, int64_t n, PcLayout* pl) {
    int rc = dudf_make_layout(cfg, n, 0, &pl->q, 1);
    if (rc) return rc;
    if (pl->q.np > (1ll << 25)) return DUDF_E_BADCFG;
    pl->chunk = n < kPcFrameChunk ? (n > 0 ? n : 1) : kPcFrameChunk;
    DudfLayout f;
    if ((rc = dudf_make_layout(cfg, pl->chunk, pl->chunk, &f, 1))) return rc;
    pl->frame_bytes = f.total_bytes;
    int64_t o = (int64_t)(pl->q.total_bytes / sizeof(float));
    auto take = [&](int64_t cnt) { int64_t r = o; o += (cnt + 63) / 64 * 64; return r; };
    pl->o_samples = take(6 * n); pl->o_prop = take(6 * n); pl->o_unit = take(6 * n); pl->o_pre = take(3 * n); pl->o_prec = take(3 * n);
    pl->o_accept = take((n + 3) / 4); pl->o_tiles = take(2 * dudf_pc_tiles(n)); pl->o_V = take(9 * pl->chunk);
    pl->o_frame = take((int64_t)(f.total_bytes / sizeof(float)));
    pl->total_bytes = (size_t)o * sizeof(float);
    return 0;
}
}  // namespace

extern "C" {

int dudf_project_points(const dudf_net_cfg* cfg, const float* theta, double* points, int64_t n, int num_steps,
                        int inverse_mode, double alpha, double surf_thresh, double* out_last_step, double* out_unit_grad,
                        float* out_pre_pos, unsigned char* out_accept, void* workspace, size_t workspace_bytes, void* stream) {
    if (inverse_mode < 0 || inverse_mode > 2 || num_steps < 1) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = dudf_launch_rays_x4(c.lo, points, c.ws, c.st))) return rc;
    return project_steps(c, theta, points, num_steps, inverse_mode, alpha, surf_thresh, out_last_step, out_unit_grad,
                         out_pre_pos, out_accept, nullptr, 0);
}

size_t dudf_pointcloud_append_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return (size_t)((2 * dudf_pc_tiles(n) * (int64_t)sizeof(int) + 255) / 256 * 256 + 256);
}

int dudf_pointcloud_append(const unsigned char* flags, int64_t n, const double* src_a, const double* src_b, const float* src_f,
                           double* dst_a, double* dst_b, float* out_f, int64_t capacity, int64_t quota, int64_t* counter,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || capacity < 0 || !counter || n > (1ll << 30)) return DUDF_E_BADCFG;
    if (!workspace || workspace_bytes < dudf_pointcloud_append_workspace_bytes(n) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return DUDF_E_WORKSPACE;
    if (n == 0) return 0;
    if (!flags || !src_a || !dst_a) return DUDF_E_BADCFG;
    return dudf_launch_pc_append(flags, n, src_a, src_b, src_f, dst_a, dst_b, out_f, capacity, quota, counter,
                                 reinterpret_cast<int*>(workspace), reinterpret_cast<hipStream_t>(stream));
}

int dudf_pointcloud_read_proposals(const dudf_net_cfg* cfg, int64_t num_points, double* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    PcLayout pl;
    int rc = make_pc_layout(cfg, num_points, &pl);
    if (rc) return rc;
    if (!workspace || workspace_bytes < pl.total_bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return DUDF_E_WORKSPACE;
    if (num_points <= 0) return 0;
    if (!out) return DUDF_E_BADCFG;
    return (int)hipMemcpyAsync(out, reinterpret_cast<float*>(workspace) + pl.o_prop, (size_t)num_points * 3 * sizeof(double),
                               hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream));
}

size_t dudf_pointcloud_workspace_bytes(const dudf_net_cfg* cfg, int64_t num_points) {
    PcLayout pl;
    if (make_pc_layout(cfg, num_points, &pl)) return 0;
    return pl.total_bytes;
}

int dudf_pointcloud_round(const dudf_net_cfg* cfg, const float* theta, int64_t num_points, int num_steps, int inverse_mode,
                          double alpha, double surf_thresh, const double* rand, int64_t rand_count, uint64_t seed, int64_t round,
                          double* surface_points, double* normals, int64_t capacity, int64_t* counter, int64_t* host_counter,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (inverse_mode < 0 || inverse_mode > 2 || num_steps < 1) return DUDF_E_BADMODE;
    PcLayout pl;
    int rc = make_pc_layout(cfg, num_points, &pl);
    if (rc) return rc;
    const int64_t n = num_points;
    if (!workspace || workspace_bytes < pl.total_bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return DUDF_E_WORKSPACE;
    if (!counter || !surface_points || !normals || capacity < 2 * n) return DUDF_E_BADCFG;
    Ctx c;
    c.lo = pl.q; c.st = reinterpret_cast<hipStream_t>(stream); c.ws = reinterpret_cast<float*>(workspace);
    hipError_t e;
    if (n > 0) {
        double* samples = reinterpret_cast<double*>(c.ws + pl.o_samples);
        double* unit = reinterpret_cast<double*>(c.ws + pl.o_unit);
        float* pre = c.ws + pl.o_pre; float* prec = c.ws + pl.o_prec;
        unsigned char* accept = reinterpret_cast<unsigned char*>(c.ws + pl.o_accept);
        const bool siren = inverse_mode == 1;
        if ((rc = dudf_launch_pc_propose(c.lo, rand, rand_count, seed, round, surface_points, counter, n, samples,
                                         reinterpret_cast<double*>(c.ws + pl.o_prop), c.ws, c.st))) return rc;
        if ((rc = project_steps(c, theta, samples, num_steps, inverse_mode, alpha, surf_thresh, nullptr, siren ? unit : nullptr,
                                siren ? nullptr : pre, accept, counter, n))) return rc;
        // accepted rows in their order behind the counter; 'siren': the unit gradients with them, otherwise the float32 pre-move
        // positions compacted as the input of the frame query
        if ((rc = dudf_launch_pc_append(accept, n, samples, siren ? unit : nullptr, siren ? nullptr : pre, surface_points,
                                        siren ? normals : nullptr, siren ? nullptr : prec, capacity, n, counter,
                                        reinterpret_cast<int*>(c.ws + pl.o_tiles), c.st))) return rc;
        if (!siren) {
            int64_t hc[4];
            if ((e = hipMemcpyAsync(hc, counter, sizeof(hc), hipMemcpyDeviceToHost, c.st)) != hipSuccess) return (int)e;
            if ((e = hipStreamSynchronize(c.st)) != hipSuccess) return (int)e;
            const int64_t added = hc[1], base = hc[2];
            if (added < 0 || base < 0 || base + added > capacity || added > n) return DUDF_E_BADCFG;
            float* V = c.ws + pl.o_V;
            for (int64_t s = 0; s < added; s += pl.chunk) {        // the Hessian sweeps run on accepted rows only
                const int64_t m = added - s < pl.chunk ? added - s : pl.chunk;
                Ctx f;
                if ((rc = dudf_make_layout(cfg, m, m, &f.lo, 1))) return rc;
                if (f.lo.total_bytes > pl.frame_bytes) return DUDF_E_WORKSPACE;
                f.st = c.st; f.ws = c.ws + pl.o_frame;
                if ((rc = forward_common(f, theta, prec + 3 * s, 0, true))) return rc;
                if ((rc = dudf_launch_field_features(f.lo, f.ws, 0, 1.0, nullptr, nullptr, nullptr, nullptr, V, f.st))) return rc;
                if ((rc = dudf_launch_pc_normals(V, m, normals + 3 * (base + s), f.st))) return rc;
            }
            if (host_counter) for (int i = 0; i < 4; ++i) host_counter[i] = hc[i];
            return 0;
        }
    }
    if (host_counter) {
        if ((e = hipMemcpyAsync(host_counter, counter, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, c.st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(c.st)) != hipSuccess) return (int)e;
    }
    return 0;
}

// ---- sphere-traced images: the entry points around dudf_trace_rays / dudf_descend_rays and the frame / curvature queries -------
int dudf_render_setup_rays(int64_t width, int64_t height, double fov, double noise, const double* rotation, const double* camera_position,
                           const double* planes, double* rays, double* t0, unsigned char* mask, void* stream) {
    if (width < 1 || height < 1 || width * height > (1ll << 30) || !rotation || !camera_position || !planes) return DUDF_E_BADCFG;
    if (!rays || !t0 || !mask) return DUDF_E_BADCFG;
    return dudf_launch_render_setup(width, height, fov, noise, rotation, camera_position, planes, rays, t0, mask,
                                    reinterpret_cast<hipStream_t>(stream));
}

int dudf_render_gather(const unsigned char* hits, int64_t m, const double* t0, const double* rays, double* out_pos, double* out_rays,
                       int32_t* out_rows, int64_t* counter, void* workspace, size_t workspace_bytes, void* stream) {
    if (m < 0 || m > (1ll << 30) || !counter) return DUDF_E_BADCFG;
    if (!workspace || workspace_bytes < dudf_pointcloud_append_workspace_bytes(m) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return DUDF_E_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(counter, 0, 4 * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    if (m == 0) return 0;
    if (!hits || !t0 || !out_pos || !out_rows || (rays && !out_rays)) return DUDF_E_BADCFG;
    int rc = dudf_launch_pc_append(hits, m, t0, rays, nullptr, out_pos, rays ? out_rays : nullptr, nullptr, m, (int64_t)1 << 62, counter,
                                   reinterpret_cast<int*>(workspace), st);
    if (rc) return rc;
    return dudf_launch_render_rows(hits, m, counter, reinterpret_cast<const int*>(workspace), out_rows, st);
}

int dudf_render_orient(const float* frame_v, const float* grad, const double* hit_rays, int64_t k, double* out_normals,
                       double* out_pc1, double* out_pc2, float* mean, void* stream) {
    if (k < 0 || (frame_v != nullptr) == (grad != nullptr) || !out_normals || (frame_v && !hit_rays)) return DUDF_E_BADCFG;
    if (k == 0) return 0;
    return dudf_launch_render_orient(frame_v, grad, hit_rays, k, out_normals, out_pc1, out_pc2, grad ? nullptr : mean,
                                     reinterpret_cast<hipStream_t>(stream));
}

int dudf_render_colormap(const float* curvatures, int64_t k, const float* bounds, const double* lut, double* out_colors, void* stream) {
    if (k < 0 || !bounds || !lut || (k > 0 && (!curvatures || !out_colors))) return DUDF_E_BADCFG;
    if (k == 0) return 0;
    return dudf_launch_render_colormap(curvatures, k, bounds, lut, out_colors, reinterpret_cast<hipStream_t>(stream));
}

int dudf_render_shade(int model, const unsigned char* hits, int64_t m, const int32_t* rows, int64_t k, const double* hit_pos,
                      const double* normals, const double* pc1, const double* pc2, const double* color_map, const double* light_position,
                      const double* camera_position, double shininess, double alpha1, double alpha2, double* accumulator, void* stream) {
    if (model != DUDF_SHADE_PHONG && model != DUDF_SHADE_WARD) return DUDF_E_BADMODE;
    if (m < 0 || k < 0 || k > m || !light_position || !accumulator || (m > 0 && !hits)) return DUDF_E_BADCFG;
    if (k > 0 && (!rows || !hit_pos || !normals)) return DUDF_E_BADCFG;
    if (model == DUDF_SHADE_WARD && (!camera_position || (k > 0 && (!pc1 || !pc2)))) return DUDF_E_BADCFG;
    if (m == 0) return 0;
    return dudf_launch_render_shade(model, hits, m, rows, k, hit_pos, normals, pc1, pc2, color_map, light_position, camera_position,
                                    shininess, alpha1, alpha2, accumulator, reinterpret_cast<hipStream_t>(stream));
}

int dudf_render_finish(const double* accumulator, int64_t count, double sample_rate, unsigned char* out_image, void* stream) {
    if (count < 0 || !(sample_rate > 0.0) || (count > 0 && (!accumulator || !out_image))) return DUDF_E_BADCFG;
    if (count == 0) return 0;
    return dudf_launch_render_finish(accumulator, count, sample_rate, out_image, reinterpret_cast<hipStream_t>(stream));
}

int dudf_grid_fields(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int64_t start, int64_t count,
                     int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (grid_n < 2 || start < 0 || count < 0 || start + count > grid_n * grid_n * grid_n) return DUDF_E_BADCFG;
    if (inverse_mode < 0 || inverse_mode > 2) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, count, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (count == 0) return 0;
    if ((rc = dudf_launch_make_x4_grid(c.lo, grid_n, start, c.ws, c.st))) return rc;
    if ((rc = forward_common(c, theta, nullptr, 0, true))) return rc;
    return dudf_launch_field_features(c.lo, c.ws, inverse_mode, alpha, out_df, out_vec, out_flag_count, nullptr,
                                      nullptr, c.st);
}

int dudf_loss_forward(const dudf_net_cfg* cfg, int mode, const float* theta, const float* x, const float* normals,
                      const float* sdf, int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights,
                      double alpha, float* out_terms, void* workspace, size_t workspace_bytes, void* stream) {
    if (mode != DUDF_LOSS_S1 && mode != DUDF_LOSS_SIREN) return DUDF_E_BADMODE;
    if (n_hess != 0 && !(mode == DUDF_LOSS_S1 && weights[2] != 0.0)) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if ((rc = forward_common(c, theta, x, 1, true))) return rc;
    return dudf_launch_loss_fwd(c.lo, mode, normals, sdf, n_global, weights, alpha, c.ws, out_terms, c.st);
}

int dudf_s2_forward_stats(const dudf_net_cfg* cfg, const float* theta, const float* x, const float* sdf,
                          int64_t n_local, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n_local, 0, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if ((rc = forward_common(c, theta, x, 1, false))) return rc;
    return dudf_launch_s2_stats(c.lo, sdf, c.ws, stats, c.st);
}

int dudf_s2_terms(const double* stats, const double* weights, float* out_terms, void* stream) {
    return dudf_launch_s2_terms(stats, weights, out_terms, reinterpret_cast<hipStream_t>(stream));
}

int dudf_loss_backward(const dudf_net_cfg* cfg, int mode, const float* theta, const float* x, const float* normals,
                       const float* sdf, int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights,
                       double alpha, const float* cot, const double* stats, float* dtheta, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (mode != DUDF_LOSS_S1 && mode != DUDF_LOSS_SIREN && mode != DUDF_LOSS_S2) return DUDF_E_BADMODE;
    if (mode == DUDF_LOSS_S2 && !stats) return DUDF_E_BADMODE;
    if (n_hess != 0 && !(mode == DUDF_LOSS_S1 && weights[2] != 0.0)) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    (void)x;
    if ((rc = dudf_launch_loss_bwd(c.lo, mode, normals, sdf, n_global, weights, alpha, cot, stats, c.ws, c.st,
                                   accumulate ? nullptr : dtheta, c.lo.n_theta)))
        return rc;
    return backward_common(c, theta, mode != DUDF_LOSS_S2, dtheta, accumulate, true);
}

int dudf_loss_backward_sweeps(const dudf_net_cfg* cfg, int mode, const float* theta, const float* normals, const float* sdf,
                              int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights, double alpha,
                              const float* cot, const double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (mode != DUDF_LOSS_S1 && mode != DUDF_LOSS_SIREN && mode != DUDF_LOSS_S2) return DUDF_E_BADMODE;
    if (mode == DUDF_LOSS_S2 && !stats) return DUDF_E_BADMODE;
    if (n_hess != 0 && !(mode == DUDF_LOSS_S1 && weights[2] != 0.0)) return DUDF_E_BADMODE;
    Ctx c;
    int rc = open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if ((rc = dudf_launch_loss_bwd(c.lo, mode, normals, sdf, n_global, weights, alpha, cot, stats, c.ws, c.st))) return rc;
    return backward_sweeps(c, theta, mode != DUDF_LOSS_S2, true);
}

int dudf_weight_gradient(const dudf_net_cfg* cfg, int64_t n_local, int64_t n_hess, int have_gradient_terms, int layer_begin,
                         int layer_end, float* dtheta, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n_local, n_hess, workspace, workspace_bytes, stream, &c);
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
    Ctx c;
    int rc = open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if ((rc = forward_common(c, theta, x, 1, true))) return rc;
    return dudf_launch_copy_out(c.lo, c.ws, out_f, out_g, nullptr, c.st);
}

int dudf_fields_backward(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n, const float* ybar,
                         const float* gbar, float* dtheta, int accumulate, void* workspace, size_t workspace_bytes,
                         void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    (void)x;
    if ((rc = dudf_launch_copy_in(c.lo, ybar, gbar, c.ws, c.st))) return rc;
    return backward_common(c, theta, gbar != nullptr, dtheta, accumulate);
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

int dudf_profile_enable(int on) {
    g_prof_on = (on != 0);
    if (g_prof_on && !g_prof_clk) {
        if (hipMalloc(&g_prof_clk, PROF_NSLOTS * 2 * sizeof(unsigned long long)) != hipSuccess) { g_prof_clk = nullptr; return 0; }
    }
    if (g_prof_on && g_prof_clk) (void)hipMemset(g_prof_clk, 0, PROF_NSLOTS * 2 * sizeof(unsigned long long));
    return 0;
}

int dudf_profile_clocks(char* buf, size_t buflen) {
    if (!g_prof_clk) { if (buflen) buf[0] = 0; return 0; }
    unsigned long long h[PROF_NSLOTS][2];
    hipError_t e = hipMemcpy(h, g_prof_clk, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    size_t off = 0;
    for (int i = 0; i < PROF_NSLOTS; ++i) {
        if (!h[i][0] || !h[i][1]) continue;
        // s_memrealtime ticks at the 100 MHz reference clock, s_memtime at the shader clock
        int w = snprintf(buf + off, off < buflen ? buflen - off : 0, "%s %.1f\n", kProfNames[i], (double)h[i][0] / (double)h[i][1] * 100.0);
        if (w < 0 || off + (size_t)w >= buflen) return DUDF_E_WORKSPACE;
        off += (size_t)w;
    }
    if (off < buflen) buf[off] = 0;
    return 0;
}

int dudf_profile_products(char* buf, size_t buflen) {
    size_t off = 0;
    for (int i = 0; i < PROF_NSLOTS; ++i) {
        if (!g_products[i]) continue;
        int w = snprintf(buf + off, off < buflen ? buflen - off : 0, "%s %d\n", kProfNames[i], g_products[i]);
        if (w < 0 || off + (size_t)w >= buflen) return DUDF_E_WORKSPACE;
        off += (size_t)w;
    }
    if (off < buflen) buf[off] = 0;
    return 0;
}

int dudf_set_option(const char* name, int value) {
    if (!name) return DUDF_E_BADMODE;
    for (int i = 0; i < OPT_COUNT; ++i)
        if (strcmp(name, kOpts[i].name) == 0) {
            if (value < kOpts[i].lo || value > kOpts[i].hi) return DUDF_E_BADCFG;
            if (i == OPT_STASH && value != 0 && value != 6 && value != 7) return DUDF_E_BADCFG;
            g_opt[i] = value;
            return 0;
        }
    return DUDF_E_BADMODE;
}

int dudf_get_option(const char* name, int* value) {
    if (!name || !value) return DUDF_E_BADMODE;
    for (int i = 0; i < OPT_COUNT; ++i)
        if (strcmp(name, kOpts[i].name) == 0) { *value = g_opt[i]; return 0; }
    return DUDF_E_BADMODE;
}

int dudf_reset_options(void) {
    for (int i = 0; i < OPT_COUNT; ++i) g_opt[i] = kOpts[i].def;
    return 0;
}

int dudf_set_wgrad_max_workgroups(int n) { return dudf_set_option("wgrad_max_workgroups", n); }

int dudf_abi_version(void) { return DUDF_ABI_VERSION; }

int dudf_profile_dump(char* buf, size_t buflen) {
    double tot[PROF_NSLOTS] = {0};
    long cnt[PROF_NSLOTS] = {0};
    for (auto& r : g_prof_recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            tot[r.slot] += ms; cnt[r.slot] += 1;
        }
        g_prof_pool.push_back(r.e0); g_prof_pool.push_back(r.e1);
    }
    g_prof_recs.clear();
    size_t off = 0;
    for (int i = 0; i < PROF_NSLOTS; ++i) {
        if (!cnt[i]) continue;
        int w = snprintf(buf + off, off < buflen ? buflen - off : 0, "%s %ld %.6f\n", kProfNames[i], cnt[i], tot[i]);
        if (w < 0 || off + (size_t)w >= buflen) return DUDF_E_WORKSPACE;
        off += (size_t)w;
    }
    if (off < buflen) buf[off] = 0;
    return 0;
}

int dudf_debug_read_stash(const dudf_net_cfg* cfg, int which, int layer, int channel, int64_t n, int64_t n_hess,
                          float* out, void* workspace, size_t workspace_bytes, void* stream) {
    Ctx c;
    int rc = open_ctx(cfg, n, n_hess, workspace, workspace_bytes, stream, &c);
    if (rc) return rc;
    if (layer < 0 || layer >= c.lo.L || channel < 0 || channel > 3) return DUDF_E_BADCFG;
    const DudfLayout& lo = c.lo;
    const int64_t offs[8] = {lo.ws_S, lo.ws_C, lo.ws_Q, lo.ws_E, lo.ws_A, lo.ws_Z, lo.ws_R, lo.ws_ZS};
    if (which < 0 || which > 7) return DUDF_E_BADMODE;
    // E, R (bit 1): 24-bit floats, tile-major; C (bit 2): 24-bit fixed point, same granules; S, Q, A, Z (bit 0): fixed point relative to
    // the column scales the sweeps leave in ws_fx
    const bool sqaz = which == 0 || which == 2 || which == 4 || which == 5;
    const int b24 = which == 7 ? 0 : which == 1 ? ((lo.p24 & 4) ? 2 : 0) : sqaz ? ((lo.p24 & 1) ? 3 : 0) : ((lo.p24 & 2) ? 1 : 0);
    const int fxi = which == 0 ? 0 : which == 2 ? 1 : which == 4 ? 2 : 3;
    return dudf_launch_read_stash(lo, c.ws + offs[which], layer, channel, out, c.st, which == 1, b24,
                                  b24 == 3 ? c.ws + lo.ws_fx[fxi] : nullptr);   // C: one copy per quad
}

int dudf_debug_stash_layout(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess, int64_t* out) {
    DudfLayout lo;
    int rc = dudf_make_layout(cfg, n, n_hess, &lo);
    if (rc) return rc;
    if (!out) return DUDF_E_BADCFG;
    const int64_t offs[8] = {lo.ws_S, lo.ws_C, lo.ws_Q, lo.ws_E, lo.ws_A, lo.ws_Z, lo.ws_R, lo.ws_ZS};
    for (int i = 0; i < 8; ++i) out[i] = offs[i] * (int64_t)sizeof(float);
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

int dudf_stash_mode(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess) {
    DudfLayout lo;
    if (dudf_make_layout(cfg, n, n_hess, &lo)) return -1;
    return lo.p24;
}

}  // extern "C"
