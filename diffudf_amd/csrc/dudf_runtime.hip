// Process-wide state behind the C ABI, host code only: the run-time options, the per-kernel HIP-event profiler, version queries.
#include "dudf_internal.h"
#include <stdio.h>
#include <string.h>
#include <vector>

// ---- run-time options (dudf_variants.h lists them).  Plain ints, read at every call: a mode switches in-process, between two steps.
namespace {
struct OptDesc { const char* name; int lo, hi; int DudfOptions::*value; };
const OptDesc kOpts[] = {
#define X(name, lo, hi, def) {#name, lo, hi, &DudfOptions::name},
    DUDF_OPTION_LIST(X)
#undef X
};
DudfOptions g_opt;
const OptDesc* find_option(const char* name) {
    for (const OptDesc& o : kOpts)
        if (strcmp(name, o.name) == 0) return &o;
    return nullptr;
}
}  // namespace

DudfOptions dudf_options() { return g_opt; }

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
int g_products[PROF_NSLOTS] = {0};
hipEvent_t prof_event() {
    if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
// the text form of the three dumps: one line per slot; line(slot, dst, room) = snprintf's result, 0 for a slot with nothing to say
template <class Line>
int dump_slots(char* buf, size_t buflen, Line line) {
    size_t off = 0;
    for (int i = 0; i < PROF_NSLOTS; ++i) {
        const int w = line(i, buf + off, off < buflen ? buflen - off : 0);
        if (w == 0) continue;
        if (w < 0 || off + (size_t)w >= buflen) return DUDF_E_WORKSPACE;
        off += (size_t)w;
    }
    if (off < buflen) buf[off] = 0;
    return 0;
}
}  // namespace

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

extern "C" {

const char* dudf_version(void) {
    return "dudf_hip 0.8 (gfx950: fp16x3 / bf16x6 MFMA sweeps and weight-gradient GEMM at fp32 accuracy, f32-input MFMA variants, "
           "Hessian quads, third-order jets, GPU sampler, ray marching, point-cloud extraction)";
}

int dudf_abi_version(void) { return DUDF_ABI_VERSION; }

int dudf_split_mode(void) { return dudf_split_mask(g_opt) | (g_opt.split ? 16 : 0); }

int dudf_set_option(const char* name, int value) {
    const OptDesc* o = name ? find_option(name) : nullptr;
    if (!o) return DUDF_E_BADMODE;
    if (value < o->lo || value > o->hi) return DUDF_E_BADCFG;
    if (o->value == &DudfOptions::stash && value != 0 && value != 6 && value != 7) return DUDF_E_BADCFG;
    g_opt.*(o->value) = value;
    return 0;
}

int dudf_get_option(const char* name, int* value) {
    const OptDesc* o = (name && value) ? find_option(name) : nullptr;
    if (!o) return DUDF_E_BADMODE;
    *value = g_opt.*(o->value);
    return 0;
}

int dudf_reset_options(void) {
    g_opt = DudfOptions();
    return 0;
}

int dudf_set_wgrad_max_workgroups(int n) { return dudf_set_option("wgrad_max_workgroups", n); }

int dudf_profile_enable(int on) {
    g_prof_on = (on != 0);
    if (g_prof_on && !g_prof_clk) {
        if (hipMalloc(&g_prof_clk, PROF_NSLOTS * 2 * sizeof(unsigned long long)) != hipSuccess) { g_prof_clk = nullptr; return 0; }
    }
    if (g_prof_on && g_prof_clk) (void)hipMemset(g_prof_clk, 0, PROF_NSLOTS * 2 * sizeof(unsigned long long));
    return 0;
}

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
    return dump_slots(buf, buflen, [&](int i, char* dst, size_t room) {
        return cnt[i] ? snprintf(dst, room, "%s %ld %.6f\n", kProfNames[i], cnt[i], tot[i]) : 0;
    });
}

int dudf_profile_clocks(char* buf, size_t buflen) {
    if (!g_prof_clk) { if (buflen) buf[0] = 0; return 0; }
    unsigned long long h[PROF_NSLOTS][2];
    hipError_t e = hipMemcpy(h, g_prof_clk, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    // s_memrealtime ticks at the 100 MHz reference clock, s_memtime at the shader clock
    return dump_slots(buf, buflen, [&](int i, char* dst, size_t room) {
        return (h[i][0] && h[i][1]) ? snprintf(dst, room, "%s %.1f\n", kProfNames[i], (double)h[i][0] / (double)h[i][1] * 100.0) : 0;
    });
}

int dudf_profile_products(char* buf, size_t buflen) {
    return dump_slots(buf, buflen, [&](int i, char* dst, size_t room) {
        return g_products[i] ? snprintf(dst, room, "%s %d\n", kProfNames[i], g_products[i]) : 0;
    });
}

}  // extern "C"
