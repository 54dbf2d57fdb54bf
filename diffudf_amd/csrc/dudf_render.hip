// Sphere-traced images on the device — the kernels around the marching loop (dudf_trace_rays / dudf_descend_rays) and the frame /
// curvature queries that replace the numpy glue of reference generate_st.py:41-101, :139 and src/render_st.py:104-114, :174-245:
// camera rays against the six box planes, the gather of the hits, orientation of the normals, the curvature colour
// map, the two reflection models with the scatter into the image, and the final 8-bit image; with the dudf_render_* entry points.
//
// The reference does all of this in float64 numpy (normals, principal directions and curvatures arrive as float32 from torch and
// are promoted where they meet a float64 operand).  Same here, operation by operation and in its order; no contraction: numpy
// rounds every product and sum.  One thread per ray or hit, rows of three consecutive values.
#include "dudf_context.h"

#include <cfloat>

namespace {

constexpr int kGridCap = 4096;                         // workgroups per launch; the kernels stride over the rest

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// reference src/util.py:34-39: arr / ||arr||, the norm as numpy's add.reduce sums it
__device__ __forceinline__ void normalize3(const double* a, double* o) {
    const double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    o[0] = a[0] / n; o[1] = a[1] / n; o[2] = a[2] / n;
}
__device__ __forceinline__ double clip09(double x) { return x < 0.0 ? 0.0 : (x > 0.9 ? 0.9 : x); }   // np.clip(., 0, 0.9): NaN stays

// ---- ray set-up (reference generate_st.py:9-33 get_pixels_camera, :63-101) ------------------------------------------------------
struct SetupArgs {
    int64_t width, height;          // get_pixels_camera's (width, height): pixel p = iy * width + ix
    double fov, noise;
    double R[9];                    // row-major camera rotation
    double cam[3];                  // rendering_config['camera_position'] as float64
    double planes[6];               // x+, x-, y+, y-, z+, z-
    double* rays; double* t0; unsigned char* mask;
};

__global__ __launch_bounds__(256) void render_setup_kernel(SetupArgs a) {
#pragma clang fp contract(off)
    const int64_t m = a.width * a.height;
    const double aspect = (double)a.width / (double)a.height;
    const double th = tan(a.fov * 3.141592653589793 / 180.0 / 2.0);
    // the reference adds the camera position as np.float32 (:44, :64) to the rotated pixel, and the python list (float64) everywhere else
    const double c32[3] = {(double)(float)a.cam[0], (double)(float)a.cam[1], (double)(float)a.cam[2]};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ix = p % a.width, iy = p / a.width;
        const double sx = 2.0 * (((double)ix + a.noise) / (double)a.width) - 1.0;
        const double sy = 2.0 * (((double)iy + a.noise) / (double)a.height) - 1.0;
        const double px[3] = {sx * aspect * th, sy * th, -1.0};
        double d[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = ((a.R[i * 3] * px[0] + a.R[i * 3 + 1] * px[1]) + a.R[i * 3 + 2] * px[2]) + c32[i];
        const double nrm = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = (d[i] / nrm) * -1.0;
        // six planes (:68-99): plane j has normal e_(j/2); numerator = offset - camera, denominator = that ray component
        bool valid = false;
        double dmin = __builtin_inf();
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double num = a.planes[j] - a.cam[j >> 1];
            const double den = d[j >> 1];
            const double ds = num / (fabs(den) < 1e-5 ? 1.0 : den);
            bool inside = true;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double q = d[i] * ds + a.cam[i];
                inside = inside && (q >= -1.001) && (q <= 1.001);
            }
            const bool ok = inside && (fabs(den) > 1e-5);
            valid = valid || ok;
            if (ok && ds >= 0.0 && ds < dmin) dmin = ds;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a.rays[p * 3 + i] = d[i];
            a.t0[p * 3 + i] = valid ? d[i] * dmin + a.cam[i] : 0.0;
        }
        a.mask[p] = valid ? 1 : 0;
    }
}

// ---- normals of the hits (reference src/render_st.py:80-83 / :101-108) ----------------------------------------------------------
// frame != nullptr: n = v_2, principal directions v_0, v_1 of the eigen-frame (float32, promoted), align = -sign(n . ray),
// n *= align, mean *= align (mean only when it is plotted).  grad != nullptr ('siren'): n = normalize(grad) in float32, no
// orientation — the reference's gradient branch has none.
__global__ __launch_bounds__(256) void render_orient_kernel(const float* __restrict__ frame, const float* __restrict__ grad,
                                                            const double* __restrict__ rays, int64_t k, double* __restrict__ normals,
                                                            double* __restrict__ pc1, double* __restrict__ pc2, float* __restrict__ mean) {
#pragma clang fp contract(off)
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < k; p += (int64_t)gridDim.x * blockDim.x) {
        if (grad) {
            const float g0 = grad[p * 3], g1 = grad[p * 3 + 1], g2 = grad[p * 3 + 2];
            const float nrm = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
            normals[p * 3] = (double)(g0 / nrm); normals[p * 3 + 1] = (double)(g1 / nrm); normals[p * 3 + 2] = (double)(g2 / nrm);
            continue;
        }
        const float* V = frame + p * 9;
        const double n[3] = {(double)V[2], (double)V[5], (double)V[8]};
        const double s = dot3(n, rays + p * 3);
        const double align = (s > 0.0 ? 1.0 : (s < 0.0 ? -1.0 : s)) * -1.0;        // np.sign: 0 for 0, NaN for NaN
        const float alignf = (float)align;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            normals[p * 3 + i] = (double)(V[i * 3 + 2] * alignf);                    // float32 in place there
            if (pc1) pc1[p * 3 + i] = (double)V[i * 3];
            if (pc2) pc2[p * 3 + i] = (double)V[i * 3 + 1];
        }
        if (mean) mean[p] = mean[p] * alignf;
    }
}

// ---- curvature colours (reference :110-114): clip to the percentile bounds, shift, scale — float32 — and look the colour up ----
__global__ __launch_bounds__(256) void render_colormap_kernel(const float* __restrict__ curv, int64_t k, const float* __restrict__ bounds,
                                                              const double* __restrict__ lut, double* __restrict__ out) {
#pragma clang fp contract(off)
    const float lo = bounds[0], hi = bounds[1];
    // after the clip the smallest value is lo and the largest hi (percentiles of the same values), so min = lo, max = hi - lo
    const float top = hi - lo;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < k; p += (int64_t)gridDim.x * blockDim.x) {
        float c = curv[p];
        c = c < lo ? lo : (c > hi ? hi : c);
        const float x = ((c - lo) / top) * 256.0f;          // matplotlib Colormap.__call__: xa *= N in the input's dtype
        if (x != x) {                                       // NaN (hi == lo): matplotlib's "bad" colour, (0, 0, 0)
            out[p * 3] = 0.0; out[p * 3 + 1] = 0.0; out[p * 3 + 2] = 0.0;
            continue;
        }
        int row = (int)x;
        row = row < 0 ? 0 : (row > 255 ? 255 : row);
        out[p * 3] = lut[row * 3]; out[p * 3 + 1] = lut[row * 3 + 1]; out[p * 3 + 2] = lut[row * 3 + 2];
    }
}

// ---- reflection models (reference :174-204 phong_shading, :206-245 ward_reflectance) and the scatter `colors[hits] = ...` --------
struct ShadeArgs {
    int model;                      // 0 blinn-phong, 1 ward
    int64_t k;
    const int* rows; const double* pos; const double* normals; const double* pc1; const double* pc2; const double* cmap;
    double light[3], camera[3];
    double shininess, alpha1, alpha2, ward_norm;        // ward_norm = 4 pi alpha1 alpha2, formed on the host in the reference's order
    double* acc;
};

__global__ __launch_bounds__(256) void render_shade_kernel(ShadeArgs a) {
#pragma clang fp contract(off)
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.k; p += (int64_t)gridDim.x * blockDim.x) {
        const double x[3] = {a.pos[p * 3], a.pos[p * 3 + 1], a.pos[p * 3 + 2]};
        const double n[3] = {a.normals[p * 3], a.normals[p * 3 + 1], a.normals[p * 3 + 2]};
        double t[3], L[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = a.light[i] - x[i];
        normalize3(t, L);
        const double ndl = dot3(n, L);
        const double lambertian = (ndl > 0.0 || ndl != ndl) ? ndl : 0.0;           // np.max([., 0]): NaN stays
        double specular;
        if (a.model == 0) {
            double I[3], R[3], V[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) I[i] = -1.0 * L[i];
            const double two_ni = 2.0 * dot3(n, I);
#pragma unroll
            for (int i = 0; i < 3; ++i) R[i] = I[i] - two_ni * n[i];
            normalize3(x, V);
            const double rv = dot3(R, V);
            const double ang = (rv > 0.0 || rv != rv) ? rv : 0.0;
            specular = (a.shininess > 0.0 && lambertian > 0.0) ? pow(ang, a.shininess) : 0.0;
        } else {
            double v[3], h[3], H[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = a.camera[i] - x[i];
            normalize3(t, v);
#pragma unroll
            for (int i = 0; i < 3; ++i) h[i] = v[i] + L[i];
            normalize3(h, H);
            const double weight = 1.0 / (a.ward_norm * sqrt(ndl * dot3(n, v)));
            const double e1 = dot3(H, a.pc1 + p * 3) / a.alpha1, e2 = dot3(H, a.pc2 + p * 3) / a.alpha2;
            specular = weight * exp((-2.0 * (e1 * e1 + e2 * e2)) / (1.0 + dot3(n, H)));
            // np.nan_to_num: NaN -> 0, +-inf -> +-DBL_MAX (the clip below then gives 0.9 or 0); then ro = 0.1
            if (specular != specular) specular = 0.0;
            else if (specular > DBL_MAX) specular = DBL_MAX;
            else if (specular < -DBL_MAX) specular = -DBL_MAX;
            specular = specular * 0.1;
        }
        const int64_t row = a.rows[p];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double dc = 0.7, sc = 0.7, ac = 0.2;
            if (a.cmap) { const double c = a.cmap[p * 3 + i]; dc = c * 0.7; sc = c * 0.7; ac = c * 0.2; }
            a.acc[row * 3 + i] += clip09((dc * lambertian + sc * specular) + ac);
        }
    }
}

// pixels without a hit keep the 1.0 of `np.ones_like(samples)`
__global__ __launch_bounds__(256) void render_background_kernel(const unsigned char* __restrict__ hits, int64_t m, double* __restrict__ acc) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x)
        if (!hits[p]) { acc[p * 3] += 1.0; acc[p * 3 + 1] += 1.0; acc[p * 3 + 2] += 1.0; }
}

// ---- (colores / sample_rate * 255).astype(np.uint8)  (reference generate_st.py:139) ---------------------------------------------
__global__ __launch_bounds__(256) void render_finish_kernel(const double* __restrict__ acc, int64_t count, double sample_rate,
                                                            unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < count; p += (int64_t)gridDim.x * blockDim.x) {
        const double v = acc[p] / sample_rate * 255.0;
        out[p] = (v != v) ? 0 : (unsigned char)(int)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));   // values lie in [0, 255]: truncation
    }
}

int dudf_launch_render_setup(int64_t width, int64_t height, double fov, double noise, const double* R, const double* cam,
                             const double* planes, double* rays, double* t0, unsigned char* mask, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    SetupArgs a;
    a.width = width; a.height = height; a.fov = fov; a.noise = noise;
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.cam[i] = cam[i];
    for (int i = 0; i < 6; ++i) a.planes[i] = planes[i];
    a.rays = rays; a.t0 = t0; a.mask = mask;
    return dudf_launch(render_setup_kernel, dim3(dudf_grid_for(width * height, 256, kGridCap)), dim3(256), st, a);
}

int dudf_launch_render_orient(const float* frame, const float* grad, const double* rays, int64_t k, double* normals, double* pc1,
                              double* pc2, float* mean, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(render_orient_kernel, dim3(dudf_grid_for(k, 256, kGridCap)), dim3(256), st, frame, grad, rays, k, normals, pc1, pc2,
                       mean);
}

int dudf_launch_render_colormap(const float* curv, int64_t k, const float* bounds, const double* lut, double* out, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(render_colormap_kernel, dim3(dudf_grid_for(k, 256, kGridCap)), dim3(256), st, curv, k, bounds, lut, out);
}

int dudf_launch_render_shade(int model, const unsigned char* hits, int64_t m, const int* rows, int64_t k, const double* pos,
                             const double* normals, const double* pc1, const double* pc2, const double* cmap, const double* light,
                             const double* camera, double shininess, double alpha1, double alpha2, double* acc, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    DUDF_TRY(dudf_launch(render_background_kernel, dim3(dudf_grid_for(m, 256, kGridCap)), dim3(256), st, hits, m, acc));
    if (k > 0) {
        ShadeArgs a;
        a.model = model; a.k = k; a.rows = rows; a.pos = pos; a.normals = normals; a.pc1 = pc1; a.pc2 = pc2; a.cmap = cmap;
        for (int i = 0; i < 3; ++i) { a.light[i] = light[i]; a.camera[i] = camera ? camera[i] : 0.0; }
        a.shininess = shininess; a.alpha1 = alpha1; a.alpha2 = alpha2;
        a.ward_norm = 4 * 3.141592653589793 * alpha1 * alpha2;
        a.acc = acc;
        DUDF_TRY(dudf_launch(render_shade_kernel, dim3(dudf_grid_for(k, 256, kGridCap)), dim3(256), st, a));
    }
    return 0;
}

int dudf_launch_render_finish(const double* acc, int64_t count, double sample_rate, unsigned char* out, hipStream_t st) {
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(render_finish_kernel, dim3(dudf_grid_for(count, 256, kGridCap)), dim3(256), st, acc, count, sample_rate, out);
}

}  // namespace

// ---- the entry points around dudf_trace_rays / dudf_descend_rays and the frame / curvature queries (dudf_query.hip) -------------
extern "C" {

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
    if (int rc = dudf_check_buffer(workspace, workspace_bytes, dudf_pointcloud_append_workspace_bytes(m))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DUDF_TRY(hipMemsetAsync(counter, 0, 4 * sizeof(int64_t), st));
    if (m == 0) return 0;
    if (!hits || !t0 || !out_pos || !out_rows || (rays && !out_rays)) return DUDF_E_BADCFG;
    // the compaction's scatter leaves the image row of every gathered hit (the index behind `colors[hits] = ...`) in out_rows
    return dudf_launch_pc_append(hits, m, t0, rays, nullptr, out_pos, rays ? out_rays : nullptr, nullptr, out_rows, m, (int64_t)1 << 62,
                                 counter, reinterpret_cast<int*>(workspace), st);
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

}  // extern "C"
