// Dense point-cloud extraction on the device — the kernels around the value+gradient sweeps and the frame query that replace
// the host loop of reference src/render_pc.py:26-73 (`Sampler.generate_point_cloud`): propose, project step, ordered
// compaction / append, normals; and the entry points that sequence them (dudf_project_points, dudf_pointcloud_*).
//
// The reference keeps the samples in float64 numpy, feeds float32 copies to the network (src/evaluate.py:18), forms the step
// with `inverse` in float64 on the float32 value WITHOUT abs (:51) and moves in float64 (:53).  Same here, operation by
// operation (no contraction: numpy rounds every product and sum).
#include "dudf_context.h"
#include "dudf_rng.h"
#include "dudf_wgscan.h"

namespace {

constexpr int kGridCap = 2048;                         // workgroups per launch; the kernels stride over the rest

// counter-based random numbers (dudf_rng.h), keyed by (seed, round, stream)
__device__ __forceinline__ double normal01(uint64_t key, uint64_t idx) {        // Box-Muller on two counters of one stream
    const double u1 = 1.0 - dudf_uniform01(key, 2 * idx), u2 = dudf_uniform01(key, 2 * idx + 1);   // u1 in (0, 1]
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// ---- propose (reference :35-39): the float64 sample rows and the padded float32 x4 of the sweep in one pass ------------------
//   held == 0 : n uniform rows;   held > 0 : n/2 rows surface[idx] + N(0, 0.1), then n/2 uniform rows (2*(n/2) rows in all: a
//   last odd row is NaN and can never be accepted).  rand != nullptr: the host's numbers (layout: include/dudf_hip.h).
__global__ __launch_bounds__(256) void pc_propose_kernel(const double* __restrict__ rand, int64_t rand_count, uint64_t key, int64_t n, int64_t np,
                                                         const double* __restrict__ surface, const int64_t* __restrict__ counter,
                                                         int64_t quota, double* __restrict__ samples, double* __restrict__ proposals,
                                                         float* __restrict__ x4) {
#pragma clang fp contract(off)
    const int64_t held = counter[0];
    if (held >= quota) return;
    const int64_t half = n / 2;
    const bool short_rand = rand && rand_count < (held ? 7 * half : 3 * n);     // never read past the host's buffer
    const int64_t m = short_rand ? 0 : (held ? 2 * half : n);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < np; p += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (p < n) {
            double q[3];
            if (p >= m) {
                q[0] = q[1] = q[2] = __builtin_nan("");
            } else if (held && p < half) {
                int64_t idx = rand ? (int64_t)rand[p] : (int64_t)(dudf_uniform01(key, (uint64_t)p) * (double)held);
                idx = idx < 0 ? 0 : (idx >= held ? held - 1 : idx);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double z = rand ? rand[half + p * 3 + k] : 0.1 * normal01(key + 1 + k, (uint64_t)p);
                    q[k] = surface[idx * 3 + k] + z;
                }
            } else {
                const int64_t r = held ? p - half : p;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    q[k] = rand ? rand[(held ? 4 * half : 0) + r * 3 + k] : dudf_uniform01(key + 4 + k, (uint64_t)p) * 2.0 - 1.0;
            }
            samples[p * 3] = q[0]; samples[p * 3 + 1] = q[1]; samples[p * 3 + 2] = q[2];
            proposals[p * 3] = q[0]; proposals[p * 3 + 1] = q[1]; proposals[p * 3 + 2] = q[2];     // kept for dudf_pointcloud_read_proposals
            if (p < m) v = f32x4{(float)q[0], (float)q[1], (float)q[2], 1.f};
        }
        *reinterpret_cast<f32x4*>(x4 + p * 4) = v;
    }
}

// ---- one projection step (reference :50-53) behind the value+gradient sweeps; writes the NEXT step's x4 itself.  The last
// step also leaves the step length, the pre-move unit gradient and float32 position, and the accept flag (:55-56).
struct PcStepArgs {
    const float* y; const float* g;       // sweep outputs: [np], [np][4]
    double* samples; float* x4;
    int64_t n;
    int inverse_mode; double alpha, inv_alpha, sqrt_alpha, thresh;
    int last;
    double* out_step; double* out_unit; float* out_pre; unsigned char* out_accept;
    const int64_t* counter; int64_t quota;     // round mode: nothing moves once the quota is reached
};

__global__ __launch_bounds__(256) void pc_step_kernel(PcStepArgs a) {
#pragma clang fp contract(off)
    if (a.counter && a.counter[0] >= a.quota) return;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * blockDim.x) {
        const double u = (double)a.y[p];
        double step;
        if (a.inverse_mode == 0) step = (u < a.inv_alpha) ? sqrt(u / a.alpha) : u;                 // 'tanh': NaN for u < 0
        else if (a.inverse_mode == 1) step = (u > 0.0) ? u : 0.0;                                  // 'siren', min_step = 0
        else step = ((u > 0.0) ? sqrt(u) : 0.0) / a.sqrt_alpha;                                    // 'squared'
        const double gx = (double)a.g[p * 4], gy = (double)a.g[p * 4 + 1], gz = (double)a.g[p * 4 + 2];
        const double nrm = sqrt(gx * gx + gy * gy + gz * gz);
        const double ux = gx / nrm, uy = gy / nrm, uz = gz / nrm;
        const double o0 = a.samples[p * 3], o1 = a.samples[p * 3 + 1], o2 = a.samples[p * 3 + 2];
        const double q0 = o0 - step * ux, q1 = o1 - step * uy, q2 = o2 - step * uz;
        a.samples[p * 3] = q0; a.samples[p * 3 + 1] = q1; a.samples[p * 3 + 2] = q2;
        if (!a.last) {
            *reinterpret_cast<f32x4*>(a.x4 + p * 4) = f32x4{(float)q0, (float)q1, (float)q2, 1.f};
        } else {
            if (a.out_step) a.out_step[p] = step;
            if (a.out_unit) { a.out_unit[p * 3] = ux; a.out_unit[p * 3 + 1] = uy; a.out_unit[p * 3 + 2] = uz; }
            if (a.out_pre) { a.out_pre[p * 3] = (float)o0; a.out_pre[p * 3 + 1] = (float)o1; a.out_pre[p * 3 + 2] = (float)o2; }
            if (a.out_accept) {
                const bool inside = q0 >= -1.0 && q0 <= 1.0 && q1 >= -1.0 && q1 <= 1.0 && q2 >= -1.0 && q2 <= 1.0;
                a.out_accept[p] = (inside && step < a.thresh) ? 1 : 0;
            }
        }
    }
}

// ---- ordered compaction + append (reference :58-65: samples[mask] / vstack) ----------------------------------------------------
// Tiles of 256 rows (one workgroup pass = 4 waves of 64).  count: accepted rows per tile (dudf_wg_rank's total);  scan: one
// workgroup turns the counts into exclusive offsets and moves the row counter;  scatter: row -> base + tile offset + accepted
// rows before it in the tile (dudf_wg_rank).  Order of the rows is kept: later rounds index the buffer.
constexpr int kTile = DUDF_WG;

__global__ __launch_bounds__(256) void pc_count_kernel(const unsigned char* __restrict__ flags, int64_t n, int64_t ntiles,
                                                       int* __restrict__ tile_cnt) {
    __shared__ unsigned wave_tot[kTile / 64];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t row = t * kTile + threadIdx.x;
        unsigned total;
        dudf_wg_rank(row < n && flags[row] != 0, wave_tot, &total);
        if (threadIdx.x == 0) tile_cnt[t] = (int)total;
    }
}

// counter: [0] rows held, [1] rows this call adds, [2] rows held before it
__global__ __launch_bounds__(256) void pc_scan_kernel(const int* __restrict__ tile_cnt, int* __restrict__ tile_off, int64_t ntiles,
                                                      int64_t capacity, int64_t quota, int64_t* __restrict__ counter) {
    __shared__ int64_t part[256];
    const int64_t per = (ntiles + 255) / 256;
    const int64_t t0 = (int64_t)threadIdx.x * per, t1 = (t0 + per < ntiles) ? t0 + per : ntiles;
    int64_t s = 0;
    for (int64_t t = t0; t < t1; ++t) s += tile_cnt[t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) { const int64_t c = part[i]; part[i] = run; run += c; }
        const int64_t held = counter[0];
        const bool ok = held < quota && held + run <= capacity;
        counter[2] = held; counter[1] = ok ? run : 0; counter[0] = held + (ok ? run : 0);
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t t = t0; t < t1; ++t) { tile_off[t] = (int)run; run += tile_cnt[t]; }
}

__global__ __launch_bounds__(256) void pc_scatter_kernel(const unsigned char* __restrict__ flags, int64_t n, int64_t ntiles,
                                                         const int* __restrict__ tile_off, const int64_t* __restrict__ counter,
                                                         const double* __restrict__ src_a, const double* __restrict__ src_b,
                                                         const float* __restrict__ src_f, double* __restrict__ dst_a,
                                                         double* __restrict__ dst_b, float* __restrict__ out_f,
                                                         int* __restrict__ rows) {
    __shared__ unsigned wave_tot[kTile / 64];
    if (counter[1] == 0) return;                   // nothing accepted, quota reached or no room: nothing is written
    const int64_t base = counter[2];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t row = t * kTile + threadIdx.x;
        const bool f = row < n && flags[row] != 0;
        unsigned total;
        const unsigned before = dudf_wg_rank(f, wave_tot, &total);
        if (f) {
            const int64_t local = (int64_t)tile_off[t] + before, d = base + local;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dst_a[d * 3 + k] = src_a[row * 3 + k];
                if (dst_b) dst_b[d * 3 + k] = src_b[row * 3 + k];
                if (out_f) out_f[local * 3 + k] = src_f[row * 3 + k];
            }
            if (rows) rows[local] = (int)row;      // local < counter[1] <= n
        }
    }
}

// ---- normals of the accepted rows from the frame query's eigenvectors: n = v_2 (reference :65, `eigh(...)[1][:, 2]`) ---------
__global__ __launch_bounds__(256) void pc_normals_kernel(const float* __restrict__ V, int64_t m, double* __restrict__ normals) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
        normals[p * 3] = (double)V[p * 9 + 2]; normals[p * 3 + 1] = (double)V[p * 9 + 5]; normals[p * 3 + 2] = (double)V[p * 9 + 8];
    }
}

int dudf_launch_pc_propose(const DudfLayout& lo, const double* rand, int64_t rand_count, uint64_t seed, int64_t round, const double* surface,
                           const int64_t* counter, int64_t quota, double* samples, double* proposals, float* ws, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    const uint64_t key = dudf_splitmix64(dudf_splitmix64(seed) ^ (uint64_t)round * 0x100000001B3ull) & ~0xFull;   // streams key + 0 .. 6
    return dudf_launch(pc_propose_kernel, dim3(dudf_grid_for(lo.np, 256, kGridCap)), dim3(256), st, rand, rand_count, key, lo.n, lo.np,
                       surface, counter, quota, samples, proposals, ws + lo.ws_x4);
}

int dudf_launch_pc_step(const DudfLayout& lo, float* ws, double* samples, int inverse_mode, double alpha, double thresh,
                        int last, double* out_step, double* out_unit, float* out_pre, unsigned char* out_accept,
                        const int64_t* counter, int64_t quota, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    PcStepArgs a;
    a.y = ws + lo.ws_y; a.g = ws + lo.ws_g; a.samples = samples; a.x4 = ws + lo.ws_x4; a.n = lo.n;
    a.inverse_mode = inverse_mode; a.alpha = alpha; a.inv_alpha = 1.0 / alpha; a.sqrt_alpha = sqrt(alpha); a.thresh = thresh;
    a.last = last; a.out_step = out_step; a.out_unit = out_unit; a.out_pre = out_pre; a.out_accept = out_accept;
    a.counter = counter; a.quota = quota;
    return dudf_launch(pc_step_kernel, dim3(dudf_grid_for(lo.n, 256, kGridCap)), dim3(256), st, a);
}

int dudf_launch_pc_normals(const float* V, int64_t m, double* normals, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(pc_normals_kernel, dim3(dudf_grid_for(m, 256, kGridCap)), dim3(256), st, V, m, normals);
}

// the projection loop of reference src/render_pc.py:43-56 on a context whose x4 already holds the float32 copies of `samples`:
// per step the value+gradient sweeps and ONE kernel (step in double, move, next x4).  The first step packs theta (dudf_forward_common);
// the later ones find the A-operand forms where it left them.  counter / quota: round mode (nothing moves once the quota is reached).
int project_steps(DudfCtx& c, const float* theta, double* samples, int num_steps, int inverse_mode, double alpha, double thresh,
                  double* out_step, double* out_unit, float* out_pre, unsigned char* out_accept, const int64_t* counter,
                  int64_t quota) {
    int rc;
    SweepArgs a = dudf_make_sweep_args(c.lo, theta, c.ws);
    a.store_c = 1;
    for (int s = 0; s < num_steps; ++s) {
        if (s == 0) {
            if ((rc = dudf_forward_common(c, theta, nullptr, 0, true))) return rc;
        } else {
            if ((rc = dudf_run_sweep(SWEEP_FWD, c.lo, a, c.st))) return rc;
            if ((rc = dudf_run_sweep(SWEEP_REV, c.lo, a, c.st))) return rc;
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
    DudfCarver cv = {(int64_t)(pl->q.total_bytes / sizeof(float))};
    pl->o_samples = cv.take(6 * n); pl->o_prop = cv.take(6 * n); pl->o_unit = cv.take(6 * n); pl->o_pre = cv.take(3 * n); pl->o_prec = cv.take(3 * n);
    pl->o_accept = cv.take((n + 3) / 4); pl->o_tiles = cv.take(2 * dudf_pc_tiles(n)); pl->o_V = cv.take(9 * pl->chunk);
    pl->o_frame = cv.take((int64_t)(f.total_bytes / sizeof(float)));
    pl->total_bytes = (size_t)cv.o * sizeof(float);
    return 0;
}

}  // namespace

int64_t dudf_pc_tiles(int64_t n) { return (n + kTile - 1) / kTile; }

// scratch: [tile counts | tile offsets], dudf_pc_tiles(n) ints each;  rows (or nullptr): the source row of every row this call adds
int dudf_launch_pc_append(const unsigned char* flags, int64_t n, const double* src_a, const double* src_b, const float* src_f,
                          double* dst_a, double* dst_b, float* out_f, int* rows, int64_t capacity, int64_t quota, int64_t* counter,
                          int* scratch, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    const int64_t ntiles = dudf_pc_tiles(n);
    int* tile_cnt = scratch; int* tile_off = scratch + ntiles;
    if (!src_b) dst_b = nullptr;
    if (!src_f) out_f = nullptr;
    DUDF_TRY(dudf_launch(pc_count_kernel, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), st, flags, n, ntiles, tile_cnt));
    DUDF_TRY(dudf_launch(pc_scan_kernel, dim3(1), dim3(256), st, tile_cnt, tile_off, ntiles, capacity, quota, counter));
    return dudf_launch(pc_scatter_kernel, dim3(dudf_grid_for(n, 256, kGridCap)), dim3(256), st, flags, n, ntiles, tile_off, counter, src_a,
                       src_b, src_f, dst_a, dst_b, out_f, rows);
}

extern "C" {

int dudf_project_points(const dudf_net_cfg* cfg, const float* theta, double* points, int64_t n, int num_steps,
                        int inverse_mode, double alpha, double surf_thresh, double* out_last_step, double* out_unit_grad,
                        float* out_pre_pos, unsigned char* out_accept, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dudf_valid_inverse_mode(inverse_mode) || num_steps < 1) return DUDF_E_BADMODE;
    DudfCtx c;
    int rc = dudf_open_ctx(cfg, n, 0, workspace, workspace_bytes, stream, &c, 1);
    if (rc) return rc;
    if (n <= 0) return 0;
    if ((rc = dudf_launch_rays_x4(c.lo, points, c.ws, c.st))) return rc;
    return project_steps(c, theta, points, num_steps, inverse_mode, alpha, surf_thresh, out_last_step, out_unit_grad,
                         out_pre_pos, out_accept, nullptr, 0);
}

size_t dudf_pointcloud_append_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return dudf_round256((size_t)(2 * dudf_pc_tiles(n)) * sizeof(int)) + 256;
}

int dudf_pointcloud_append(const unsigned char* flags, int64_t n, const double* src_a, const double* src_b, const float* src_f,
                           double* dst_a, double* dst_b, float* out_f, int64_t capacity, int64_t quota, int64_t* counter,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || capacity < 0 || !counter || n > (1ll << 30)) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_pointcloud_append_workspace_bytes(n))) return rc;
    if (n == 0) return 0;
    if (!flags || !src_a || !dst_a) return DUDF_E_BADCFG;
    return dudf_launch_pc_append(flags, n, src_a, src_b, src_f, dst_a, dst_b, out_f, nullptr, capacity, quota, counter,
                                 reinterpret_cast<int*>(workspace), reinterpret_cast<hipStream_t>(stream));
}

int dudf_pointcloud_read_proposals(const dudf_net_cfg* cfg, int64_t num_points, double* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    PcLayout pl;
    int rc = make_pc_layout(cfg, num_points, &pl);
    if (rc) return rc;
    if ((rc = dudf_check_buffer(workspace, workspace_bytes, pl.total_bytes))) return rc;
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
    if (!dudf_valid_inverse_mode(inverse_mode) || num_steps < 1) return DUDF_E_BADMODE;
    PcLayout pl;
    int rc = make_pc_layout(cfg, num_points, &pl);
    if (rc) return rc;
    const int64_t n = num_points;
    if ((rc = dudf_check_buffer(workspace, workspace_bytes, pl.total_bytes))) return rc;
    if (!counter || !surface_points || !normals || capacity < 2 * n) return DUDF_E_BADCFG;
    DudfCtx c = dudf_ctx_at(pl.q, reinterpret_cast<float*>(workspace), reinterpret_cast<hipStream_t>(stream));
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
                                        siren ? normals : nullptr, siren ? nullptr : prec, nullptr, capacity, n, counter,
                                        reinterpret_cast<int*>(c.ws + pl.o_tiles), c.st))) return rc;
        if (!siren) {
            int64_t hc[4];
            DUDF_TRY(hipMemcpyAsync(hc, counter, sizeof(hc), hipMemcpyDeviceToHost, c.st));
            DUDF_TRY(hipStreamSynchronize(c.st));
            const int64_t added = hc[1], base = hc[2];
            if (added < 0 || base < 0 || base + added > capacity || added > n) return DUDF_E_BADCFG;
            float* V = c.ws + pl.o_V;
            for (int64_t s = 0; s < added; s += pl.chunk) {        // the Hessian sweeps run on accepted rows only
                const int64_t m = added - s < pl.chunk ? added - s : pl.chunk;
                DudfLayout fl;
                if ((rc = dudf_make_layout(cfg, m, m, &fl, 1))) return rc;
                if (fl.total_bytes > pl.frame_bytes) return DUDF_E_WORKSPACE;
                DudfCtx f = dudf_ctx_at(fl, c.ws + pl.o_frame, c.st);
                if ((rc = dudf_forward_common(f, theta, prec + 3 * s, 0, true))) return rc;
                if ((rc = dudf_launch_field_features(f.lo, f.ws, 0, 1.0, nullptr, nullptr, nullptr, nullptr, V, f.st))) return rc;
                if ((rc = dudf_launch_pc_normals(V, m, normals + 3 * (base + s), f.st))) return rc;
            }
            if (host_counter) for (int i = 0; i < 4; ++i) host_counter[i] = hc[i];
            return 0;
        }
    }
    if (host_counter) {
        DUDF_TRY(hipMemcpyAsync(host_counter, counter, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
        DUDF_TRY(hipStreamSynchronize(c.st));
    }
    return 0;
}

}  // extern "C"
