// What the units with C-ABI entry points share to run sweeps on a caller's workspace: the context, the sweep sequencing
// (bodies: dudf_api.hip) and the argument checks every entry point writes the same way.  Internal, host code only.
#pragma once
#include "dudf_internal.h"

// ---- the shared argument checks ------------------------------------------------------------------------------------------------
// a caller's scratch buffer: there, large enough, 256-byte aligned
inline int dudf_check_buffer(const void* ptr, size_t have, size_t need) {
    return (!ptr || have < need || (reinterpret_cast<uintptr_t>(ptr) & 255)) ? DUDF_E_WORKSPACE : 0;
}
// Carves typed arrays out of such a buffer, each on a 256-byte granule and at least one element long; base == nullptr: sizes only
// (null pointers, `o` the byte count).  A stage's carve_* function is *_workspace_bytes() on a null base and the kernels' pointers
// on the caller's: one statement of the layout.  Host glue, so it stands beside the check of the buffer it carves; DudfCarver
// (dudf_internal.h) hands out the float OFFSETS of the network layout, which kernel arguments carry.
struct DudfByteCarver {
    char* base; size_t o;
    template <class T> T* take(int64_t count) {
        T* p = base ? reinterpret_cast<T*>(base + o) : nullptr;
        o += dudf_round256((size_t)(count > 0 ? count : 1) * sizeof(T));
        return p;
    }
};
inline DudfByteCarver dudf_carve(const void* base) { return DudfByteCarver{static_cast<char*>(const_cast<void*>(base)), 0}; }
// 0 'tanh', 1 'siren', 2 'squared' (reference src/inverses.py)
inline bool dudf_valid_inverse_mode(int inverse_mode) { return !(inverse_mode < 0 || inverse_mode > 2); }

inline bool dudf_use_bf16_sweeps() { return dudf_options().sweep_family != 0; }   // 0: the f32-input MFMA kernel everywhere (A/B testing)

// ---- launches and runtime calls, checked where they are made -------------------------------------------------------------------
// a kernel with at most the default 64 KiB of dynamic LDS (the sweeps, which raise that limit, go through dudf_launch_kernel): the
// launch's own error, 0 = launched
template <class Kernel, class... Args>
inline int dudf_launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return (int)hipGetLastError();
}
// ... with none: every other launch of the geometry units
template <class Kernel, class... Args>
inline int dudf_launch(Kernel kernel, dim3 grid, dim3 block, hipStream_t st, const Args&... args) {
    return dudf_launch_lds(kernel, grid, block, 0, st, args...);
}
// leaves the entry point with the first non-zero result of a dudf_launch, a hipMemsetAsync / hipMemcpyAsync / hipStreamSynchronize or
// any other int-returning step: nothing after a failure is enqueued
#define DUDF_TRY(call) do { if (const int rc_ = (int)(call)) return rc_; } while (0)

// ---- a layout on a workspace and a stream ----------------------------------------------------------------------------------------
struct DudfCtx {
    DudfLayout lo;
    hipStream_t st;
    float* ws;
};
// layout of (cfg, n, n_h) + the check of the caller's workspace against it
int dudf_open_ctx(const dudf_net_cfg* cfg, int64_t n, int64_t n_h, void* workspace, size_t bytes, void* stream, DudfCtx* c,
                  int query_only = 0);
// a context on a layout the caller made and checked itself, `ws` somewhere inside a larger buffer
inline DudfCtx dudf_ctx_at(const DudfLayout& lo, float* ws, hipStream_t st) { return DudfCtx{lo, st, ws}; }

// ---- sweep sequencing --------------------------------------------------------------------------------------------------------------
SweepArgs dudf_make_sweep_args(const DudfLayout& lo, const float* theta, float* ws);
// one column range of a sweep: build the request, choose, note the products, launch
int dudf_launch_range(int which, int H, SweepArgs a, hipStream_t st);
// one sweep over both column ranges: Hessian quads and plain columns in one grid where a pair kernel is built (a training batch
// with Hessian-path points), otherwise the quads first, then the plain columns
int dudf_run_sweep(int base, const DudfLayout& lo, SweepArgs a, hipStream_t st);
// pack + x4 + forward (+ reverse) sweeps with the given stash flags.  x == nullptr: x4 was already filled (grid query).
// `train` = keep what the adjoint sweeps need; the forward sweep always runs its stash-everything variant (the only
// one the register allocator handles without spills), queries merely skip the reverse sweep's stores.
int dudf_forward_common(DudfCtx& c, const float* theta, const float* x, int train, bool reverse);
// the adjoint sweeps; the weight gradients follow (all layers at once, or layer ranges through dudf_weight_gradient)
int dudf_backward_sweeps(DudfCtx& c, const float* theta, int have_g, bool zeroed = false);
// `zeroed`: the caller's cotangent kernel (loss_bwd) already cleared d(theta) and the running maxima on its way
int dudf_backward_common(DudfCtx& c, const float* theta, int have_g, float* dtheta, int accumulate, bool zeroed = false);
