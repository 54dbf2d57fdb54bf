/* dudf_hip.h — C ABI of the MI355X-native DiffUDF training hot path (libdudf_hip.so).
 *
 * The reference (LIA-DiTella/DiffUDF) has no FFI: its hot path is a Python-level operator
 * API on PyTorch autograd.  Each entry point below names the reference interface it replaces
 * (file:line in the reference tree); the Python mirror in diffudf_amd/ binds them with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory unless it says "host";
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it;
 *   - no allocation inside: the caller passes a workspace of dudf_workspace_bytes() bytes,
 *     256-byte aligned (so that stash rows start on cache-line boundaries), and must leave it untouched between a *_forward and its *_backward;
 *   - return value: 0 = ok, >0 = hipError_t of a failed launch, <0 = DUDF_E_* below;
 *   - theta = flat fp32 parameters in the reference's state_dict order
 *     (net.0.0.weight (H,3) row-major, net.0.0.bias (H), net.1.0.weight (H,H), ...,
 *      net.L.0.weight (1,H), net.L.0.bias (1))  — reference src/model.py:94-113;
 *   - points are fp32: x (n,3) row-major, normals (n,3), sdf (n) — the tensors
 *     reference src/dataset.py:170-185 yields (without their leading batch-of-1 axis).
 */
#ifndef DUDF_HIP_H
#define DUDF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI number of this header; dudf_abi_version() returns the one the library was built with.  A caller built against another
 * header must not call the library: dudf_net_cfg grew by `ww` in ABI 5, dudf_stash_mode took (n, n_hess) and the options arrived in
 * ABI 6, the point-cloud calls (dudf_project_points .. dudf_pointcloud_round) in ABI 8.  The Python mirror checks it when it loads the library (diffudf_amd/_lib.py). */
#define DUDF_ABI_VERSION 8
int dudf_abi_version(void);

#define DUDF_E_BADCFG   (-1)   /* unsupported network shape: `hidden` must be one of {32,64,128,256,512} (the Python mirror pads any
                                  list of widths <= 512 to the next built width with zero units, which is exact for a sine MLP) */
#define DUDF_E_WORKSPACE (-2)  /* workspace too small / misaligned */
#define DUDF_E_BADMODE  (-3)
#define DUDF_E_UNSUPPORTED (-4)

/* loss selector — reference src/loss_functions.py:123 (loss_s1), :106 (loss_s2), :82 (loss_siren) */
#define DUDF_LOSS_S1    0
#define DUDF_LOSS_S2    1
#define DUDF_LOSS_SIREN 2

typedef struct dudf_net_cfg {
    int32_t n_in;            /* 3 */
    int32_t n_hidden_layers; /* L = len(hidden_layer_config), reference src/model.py:94-108 */
    int32_t hidden;          /* H, all hidden layers equal */
    float   w0;              /* frequency of the FIRST SineLayer, reference src/model.py:25-30, :100 */
    float   ww;              /* frequency of the other SineLayers (reference src/model.py:89-92, :103-106); 0 = the same as w0
                                (round 4, ABI 0.5: the struct grew by this field).  sin(w0 (W_1 x + b_1)) = sin(ww (rho W_1 x + rho b_1))
                                with rho = w0 / ww: the kernels run ONE frequency, ww, on a first layer scaled by rho when its
                                A-operand forms are packed, and the first layer's gradient is scaled by rho on its way out */
} dudf_net_cfg;

/* number of floats in theta for this cfg (461 825 for 8x256) */
int64_t dudf_theta_count(const dudf_net_cfg* cfg);

/* bytes of workspace needed for a local batch of n points (training: stash of all sweeps);
 * the _hess form when the first n_hess of them take the Hessian path (4 columns each instead of 1) */
size_t dudf_workspace_bytes(const dudf_net_cfg* cfg, int64_t n);
size_t dudf_workspace_bytes_hess(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess);
/* the smaller workspace that dudf_query / dudf_query_hessian / dudf_query_frame / dudf_grid_fields need
 * (n_hess = n for the Hessian/frame queries, 0 otherwise) */
size_t dudf_workspace_bytes_query(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess);

/* Replaces `model(x)['model_out']` + `gradient(y, x)` as used by the chunk loop of
 * reference src/evaluate.py:26-35 (SIREN.forward src/model.py:116-135; gradient
 * src/diff_operators.py:208-212).  out_f (n); out_g (n,3) or NULL for value only. */
int dudf_query(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
               float* out_f, float* out_g, void* workspace, size_t workspace_bytes, void* stream);

/* Value, df/dx and the Hessian d2f/dx_i dx_k of every point — replaces `model(x)`, `gradient(y,x)` and
 * `hessian(y,x)` of the chunk loop in reference src/evaluate.py:26-35 (hessian: src/diff_operators.py:187-193,
 * rows h_i = grad(g[:,i], x)).  Forward-over-reverse with three tangent channels (8 F0 flops per point).
 * out_h (n,3,3) row-major [i][k]; workspace of dudf_workspace_bytes_hess(cfg, n, n). */
int dudf_query_hessian(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
                       float* out_f, float* out_g, float* out_h, void* workspace, size_t workspace_bytes,
                       void* stream);

/* dudf_query_hessian plus the eigen-frame of the Hessian's lower triangle: out_lambda (n,3) ascending, out_v (n,3,3)
 * eigenvectors as columns ([i][j] = component i of v_j; sign arbitrary) — `torch.linalg.eigh(hessian(y,x))` as used by
 * reference src/render_st.py:57-62 `compute_normals_and_cd` (normal = v_2) and src/render_mc.py:77-78.  Any output
 * pointer may be NULL. */
int dudf_query_frame(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
                     float* out_f, float* out_g, float* out_h, float* out_lambda, float* out_v,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Normals and curvatures at query points — replaces `compute_normals_and_cd` + `compute_curvature` (reference
 * src/render_st.py:57-62, :42-55): eigh of the Hessian (normal n = v_2, principal directions v_0, v_1), the shape operator
 * J = jacobian(n, x) (src/diff_operators.py:214-227; third derivatives of f), mean = trace(J)/2,
 * gaussian = -det [[J, n],[n^T, 0]].  The sign of n — and with it of J and of the mean curvature — is arbitrary, as it
 * is for torch.linalg.eigh; the reference re-orients both afterwards (:104-108).
 * out_shape (n,3,3) row-major [i][k] = dn_i/dx_k.  One 16-column third-order Taylor jet per point on top of the
 * Hessian query (24 F0 flops per point).  Every built width (32 .. 512).  Any output may be NULL. */
size_t dudf_workspace_bytes_curvature(const dudf_net_cfg* cfg, int64_t n);
int dudf_query_curvature(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
                         float* out_lambda, float* out_v, float* out_mean, float* out_gauss, float* out_shape,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Sphere tracing on the device — replaces the loop of `propagate_rays` (reference src/render_st.py:136-161: per iteration
 * a value-only `evaluate`, `inverse(gt_mode, |f|, alpha)` (src/inverses.py), `t0 += rays * steps`, threshold / in-domain
 * masks, one D2H copy) for m rays.  rays (m,3) and t0 (m,3) are float64 like the reference's numpy arrays (the network
 * sees float32 copies, the step is taken in float32 and added in float64); mask (m) 0/1 bytes = `mask_rays` in/out,
 * hits (m) 0/1 bytes out.  The active-ray count is read back only every `check_every` iterations; iterations past the
 * point where no ray is active change nothing.  *iterations_done (host) = iterations executed.  The reference raises if
 * no ray hit; the caller checks hits.  inverse_mode 0 'tanh' / 1 'siren' / 2 'squared'; min_step = 0.01 there.
 * workspace: dudf_workspace_bytes_query(cfg, m, 0). */
int dudf_trace_rays(const dudf_net_cfg* cfg, const float* theta, const double* rays, double* t0, unsigned char* mask,
                    unsigned char* hits, int64_t m, int inverse_mode, double alpha, double min_step,
                    double surface_threshold, int max_iterations, int check_every, int* iterations_done,
                    void* workspace, size_t workspace_bytes, void* stream);
/* `grad_descent` (reference src/render_st.py:163-172): gd_steps times  t0[hits] -= normalize(grad f) * inverse(|f|). */
int dudf_descend_rays(const dudf_net_cfg* cfg, const float* theta, double* t0, const unsigned char* hits, int64_t m,
                      int inverse_mode, double alpha, double min_step, int gd_steps, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Dense oriented point cloud — replaces `Sampler.generate_point_cloud` (reference src/render_pc.py:26-73).
 *
 * dudf_project_points: the deterministic inner loop (:43-56) for n float64 points, in place: num_steps (>= 1) times
 *   udf, grad = evaluate(float32 copy of the points)                         (:46-50, src/evaluate.py:18)
 *   step = inverse(gt_mode, udf, alpha, min_step = 0)  — NO abs, in float64 on the float32 value (:51, src/inverses.py:3-21);
 *          'tanh' with udf < 0 gives NaN, which propagates into the point and fails the domain test, as it does there
 *   points -= step * normalize(grad)                                         (:53, src/util.py:34-39), float64
 * and after the last step  accept = all(-1 <= moved point <= 1) and last step < surf_thresh  (:55-56).
 * out_last_step (n) double; out_unit_grad (n,3) double = normalize(grad) at the position BEFORE the last move (the normal of
 * gt_mode 'siren', :63); out_pre_pos (n,3) float = that position as the network saw it (where the reference's Hessian of :46 was
 * evaluated); out_accept (n) 0/1 bytes.  Any output may be NULL.  inverse_mode 0 'tanh' / 1 'siren' / 2 'squared'.
 * workspace: dudf_workspace_bytes_query(cfg, n, 0). */
int dudf_project_points(const dudf_net_cfg* cfg, const float* theta, double* points, int64_t n, int num_steps,
                        int inverse_mode, double alpha, double surf_thresh, double* out_last_step, double* out_unit_grad,
                        float* out_pre_pos, unsigned char* out_accept, void* workspace, size_t workspace_bytes, void* stream);

/* Ordered append — replaces `surface_points = np.vstack((surface_points, samples[mask]))` and the same for the normals
 * (reference src/render_pc.py:58-65): the rows of src_a (n,3) double, src_b (n,3) double and src_f (n,3) float whose flag is
 * non-zero are appended IN THEIR ORDER (stable compaction: wave ballots, per-workgroup counts, a scan, a scatter) to dst_a / dst_b
 * (capacity rows) behind the device row counter, and to out_f from its row 0.  counter (device, 4 x int64): [0] rows held
 * (in/out), [1] rows this call added, [2] rows held before it, [3] unused.  A call that finds counter[0] >= quota, or whose rows
 * would not fit into `capacity`, adds nothing ([1] = 0).  Any of src_b / dst_b, src_f / out_f may be NULL; n = 0 launches nothing
 * (and leaves the counter alone).  workspace: dudf_pointcloud_append_workspace_bytes(n), 256-byte aligned. */
size_t dudf_pointcloud_append_workspace_bytes(int64_t n);
int dudf_pointcloud_append(const unsigned char* flags, int64_t n, const double* src_a, const double* src_b, const float* src_f,
                           double* dst_a, double* dst_b, float* out_f, int64_t capacity, int64_t quota, int64_t* counter,
                           void* workspace, size_t workspace_bytes, void* stream);

/* One round of the reference's outer loop (src/render_pc.py:33-68) on a caller-owned state: surface_points, normals
 * (capacity >= 2 * num_points rows of 3 doubles; a round adds at most num_points) and counter (device, 4 x int64 as above, zeroed
 * by the caller before the first round).
 *   propose : counter[0] == 0: num_points uniform rows in [-1,1]^3 (:39); otherwise num_points/2 rows gathered from ALL surface
 *             rows held, index = uniform(0, rows) truncated, plus N(0, 0.1) noise, then num_points/2 uniform rows (:36-37).
 *             rand != NULL (device, float64): the numbers the host drew in the reference's call order — (num_points,3) uniforms
 *             in the first form; [num_points/2 indices (already truncated, as doubles) | (num_points/2,3) noise |
 *             (num_points/2,3) uniforms] in the second; rand_count = how many doubles it holds (a buffer too short for the form
 *             the counter selects proposes nothing: every row of that round is NaN and rejected).  rand == NULL: a counter-based generator in the kernel, a pure function
 *             of (seed, round, row).
 *   project : dudf_project_points on those rows;  append: dudf_pointcloud_append with quota = num_points;
 *   normals : normalize(grad) for inverse_mode 1 ('siren', :63), otherwise the eigenvector of the largest Hessian eigenvalue at
 *             the pre-move position (:65) — dudf_query_frame's v_2, for the ACCEPTED rows only, in chunks.
 * A round issued when counter[0] >= num_points changes nothing.  host_counter (host, 4 x int64) or NULL: the counter after the
 * round.  The Hessian path needs the accepted count on the host to size its sweeps, so the call synchronises the stream once
 * unless inverse_mode == 1 and host_counter == NULL (then it only enqueues).  num_points = 0 is valid and launches nothing.
 * workspace: dudf_pointcloud_workspace_bytes(cfg, num_points); 0 for a refused cfg. */
size_t dudf_pointcloud_workspace_bytes(const dudf_net_cfg* cfg, int64_t num_points);
int dudf_pointcloud_round(const dudf_net_cfg* cfg, const float* theta, int64_t num_points, int num_steps, int inverse_mode,
                          double alpha, double surf_thresh, const double* rand, int64_t rand_count, uint64_t seed, int64_t round,
                          double* surface_points, double* normals, int64_t capacity, int64_t* counter, int64_t* host_counter,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Test/diagnostic hook: the rows the last round on this workspace PROPOSED (reference src/render_pc.py:36-39, before any move),
 * out (num_points,3) double. */
int dudf_pointcloud_read_proposals(const dudf_net_cfg* cfg, int64_t num_points, double* out, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* Sphere-traced images — the stages of reference generate_st.py / src/render_st.py `create_projectional_image` around the marching
 * loop and the queries above.  Everything is float64 like the reference's numpy arrays, evaluated in its order of operations
 * (no contraction); normals, principal directions and curvatures are the float32 values torch hands it, promoted where they meet
 * a float64 operand.  These entry points arrived after ABI 8 without changing any existing signature.
 *
 * dudf_render_setup_rays — generate_st.py:9-33 (`get_pixels_camera`) and :63-101 for width * height pixels, pixel p = iy * width + ix
 *   (`width`, `height` are get_pixels_camera's arguments; the reference passes its config's height and width in this order, :42).
 *   noise: the jitter of this pass; rotation (host, 9 doubles, row-major R of :49-61, formed by the caller); camera_position (host, 3
 *   doubles; the kernel adds its float32 rounding to the rotated pixel as :44/:64 do and uses the doubles for the planes); planes
 *   (host, 6 doubles, :76).  Per ray and plane: ds = numerator / (|denominator| < 1e-5 ? 1 : denominator), the intersection must lie
 *   in [-1.001, 1.001]^3 with |denominator| > 1e-5; a ray with such a plane is valid and starts at the smallest ds >= 0 of them.
 *   rays (m,3), t0 (m,3) doubles (t0 = 0 for invalid rays), mask (m) 0/1 bytes: the arguments of `create_projectional_image`. */
int dudf_render_setup_rays(int64_t width, int64_t height, double fov, double noise, const double* rotation, const double* camera_position,
                           const double* planes, double* rays, double* t0, unsigned char* mask, void* stream);

/* dudf_render_gather — `t0[hits]`, `rays[hits]` (src/render_st.py:78, :104) through dudf_pointcloud_append's ordered compaction, plus
 * the inverse map: out_rows (k) = the ray index of every gathered row, which `colors[hits] = ...` (:199, :240) scatters by.
 * counter (device, 4 x int64) is zeroed first; [1] = k afterwards.  rays / out_rays may be NULL.  out_pos, out_rays, out_rows hold m
 * rows.  workspace: dudf_pointcloud_append_workspace_bytes(m), 256-byte aligned. */
int dudf_render_gather(const unsigned char* hits, int64_t m, const double* t0, const double* rays, double* out_pos, double* out_rays,
                       int32_t* out_rows, int64_t* counter, void* workspace, size_t workspace_bytes, void* stream);

/* dudf_render_orient — src/render_st.py:101-108 for k hits: frame_v (k,3,3) from dudf_query_frame / dudf_query_curvature: normal = v_2,
 * out_pc1 / out_pc2 = v_0 / v_1 (may be NULL), align = -sign(normal . ray) with sign(0) = 0, normal *= align and, when `mean` (k,
 * in/out, the mean curvature of the SAME query) is given, mean *= align.  grad (k,3) instead of frame_v ('siren', :80-83):
 * normal = normalize(grad) in float32, not oriented.  Exactly one of frame_v / grad. */
int dudf_render_orient(const float* frame_v, const float* grad, const double* hit_rays, int64_t k, double* out_normals,
                       double* out_pc1, double* out_pc2, float* mean, void* stream);

/* dudf_render_colormap — src/render_st.py:111-114 behind the percentiles: bounds (device, 2 floats) = the two np.percentile values;
 * clip, subtract the minimum, divide by the maximum in float32, then the look-up `cmap(x)[:, :3]`: row min(int(x * 256), 255) of
 * lut (device, 256 x 3 doubles; the reference takes matplotlib's RdYlBu); NaN (both bounds equal) gives (0,0,0).
 * out_colors (k,3) doubles. */
int dudf_render_colormap(const float* curvatures, int64_t k, const float* bounds, const double* lut, double* out_colors, void* stream);

/* dudf_render_shade — `phong_shading` (src/render_st.py:174-204) or `ward_reflectance` (:206-245) for k hits and the scatter into
 * the image: accumulator (m,3) doubles += the colour at row rows[i] for every hit, += 1.0 at the pixels whose hits byte is 0
 * (`np.ones_like(samples)`; `colores +=` of generate_st.py:104, :127).  hit_pos, normals (k,3); pc1, pc2 (k,3, Ward only); color_map
 * (k,3) or NULL (0.7 / 0.7 / 0.2 grey); light_position, camera_position (host, 3 doubles; the camera for Ward only).  Phong: specular
 * only where lambertian > 0 and shininess > 0.  Ward keeps np.nan_to_num's outcome: a NaN weight gives 0, +-inf gives +-DBL_MAX,
 * which the clip to [0, 0.9] turns into 0.9 or 0. */
#define DUDF_SHADE_PHONG 0
#define DUDF_SHADE_WARD  1
int dudf_render_shade(int model, const unsigned char* hits, int64_t m, const int32_t* rows, int64_t k, const double* hit_pos,
                      const double* normals, const double* pc1, const double* pc2, const double* color_map, const double* light_position,
                      const double* camera_position, double shininess, double alpha1, double alpha2, double* accumulator, void* stream);

/* dudf_render_finish — `(colores / sample_rate * 255).astype(np.uint8)` (generate_st.py:139) over `count` doubles. */
int dudf_render_finish(const double* accumulator, int64_t count, double sample_rate, unsigned char* out_image, void* stream);

/* Chamfer distance and normal consistency — the device side of reference cuantitative.py:10-19 (`pytorch3d.loss.chamfer_distance`;
 * pytorch3d is a CUDA extension) and of :99-100 (open3d's vertex normals).  csrc/dudf_chamfer.hip.  These entry points arrived after
 * ABI 8 without changing any existing signature.
 *
 * dudf_nearest_points — for every row of x (n,3) the nearest row of y (m,3), both fp32: the `dists` / `idx` of pytorch3d's
 *   `knn_points(x, y, norm=norm, K=1)`.  norm 2: out_dist (n) = SQUARED Euclidean distance; norm 1: the L1 distance sum |x_i - y_i|.
 *   out_idx (n) int64 = the row of y.  Either output may be NULL.  Distances are formed from the differences, (x - y) then square or
 *   abs, in fp32 — never from |x|^2 + |y|^2 - 2 x.y, which cancels.  Among rows of y at equal fp32 distance the smallest index wins;
 *   the result does not depend on launch geometry or execution order, and two calls on the same inputs are bit-identical.  Inputs are
 *   expected finite: a row of x with a NaN gets a NaN distance and an index in [0, m); NaN rows of y are never chosen.
 *   norm not in {1, 2}: DUDF_E_BADMODE; n == 0: nothing is launched, 0; m <= 0 with n > 0: DUDF_E_BADCFG; n or m >= 2^31:
 *   DUDF_E_UNSUPPORTED; workspace: dudf_nearest_workspace_bytes(n) (one 64-bit key per row), 256-byte aligned, else DUDF_E_WORKSPACE. */
size_t dudf_nearest_workspace_bytes(int64_t n);
int dudf_nearest_points(const float* x, int64_t n, const float* y, int64_t m, int norm, float* out_dist, int64_t* out_idx,
                        void* workspace, size_t workspace_bytes, void* stream);

/* dudf_chamfer_terms — the two sums behind chamfer_distance's mean reductions for one direction: out_sums (device, 2 doubles) =
 *   sum_p dist[p]  and  sum_p (1 - |cos(x_normals[p], y_normals[idx[p]])|),  cos = a.b / (max(|a|, 1e-6) max(|b|, 1e-6))
 *   (`F.cosine_similarity(..., eps=1e-6)`; pytorch3d's `abs_cosine=True` normal term).  dist (n) fp32 and idx (n) int64 as
 *   dudf_nearest_points wrote them; normals fp32 (n,3) / (m,3).  Both normals NULL: only out_sums[0] is written (one of them NULL:
 *   DUDF_E_BADCFG).  An idx outside [0, m) is not dereferenced and turns the normal sum into NaN.  Accumulated in double in a fixed
 *   order — per-workgroup partials in the workspace, added in index order by one workgroup — so a repeated call is bit-identical;
 *   no floating-point atomics.  workspace: dudf_chamfer_terms_workspace_bytes(n). */
size_t dudf_chamfer_terms_workspace_bytes(int64_t n);
int dudf_chamfer_terms(const float* dist, const int64_t* idx, int64_t n, const float* x_normals, const float* y_normals, int64_t m,
                       double* out_sums, void* workspace, size_t workspace_bytes, void* stream);

/* dudf_vertex_normals — open3d's `compute_vertex_normals(normalized=True)` (reference cuantitative.py:99-100): every face adds its
 *   unnormalised (v1 - v0) x (v2 - v0) to its three vertices (area weighting), then each sum is normalised.  vertices (V,3) double,
 *   faces (F,3) int64, out_normals (V,3) fp32.  A vertex with a zero sum gets (0, 0, 1); a face with an index outside [0, V) is
 *   skipped, not dereferenced.  Sums in double (atomic adds into the workspace; their order moves the sum by ~1e-16 relative, which
 *   the rounding to fp32 hides except at a rounding boundary).  workspace: dudf_vertex_normals_workspace_bytes(V). */
size_t dudf_vertex_normals_workspace_bytes(int64_t n_vertices);
int dudf_vertex_normals(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, float* out_normals,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Surface-sampled evaluation — an area-uniform sampler of a triangle mesh and the threshold statistics of a distance vector, what
 * `diffudf_amd.metrics.surface_metrics` (Chamfer distance on surface samples, F-score, Hausdorff) is made of.
 * csrc/dudf_surfsample.hip; the rules are DESIGN.md §8 (tests/surface_oracle.py restates them in numpy).  These entry points arrived
 * after ABI 8 without changing any existing signature.
 *
 * dudf_mesh_sample_surface — n samples with global indices start .. start + n - 1 of the mesh vertices (V,3) double, faces (F,3)
 *   int64.  Per face in fp64: n = (b - a) x (c - a), each component two products and one difference; nn = sqrt((nx^2 + ny^2) + nz^2);
 *   the face normal is n / max(nn, 1e-300) rounded to fp32 (out_face_normals (F,3), or NULL); out_area (device, 1 double, or NULL) =
 *   0.5 * sum nn from per-workgroup partials added in index order.  Faces are chosen by INTEGER weights w_f = floor(nn_f / nn_max *
 *   2^32) with nn_max the maximum over the faces, c_f their inclusive uint64 sums, W = c_{F-1}: integer sums are the same in every
 *   order.  A face of weight 0 (degenerate, or below 2^-32 of the largest) is never chosen.  Sample g draws 64-bit words b1, b2, b3
 *   from streams 301, 302, 303 of `seed` (the splitmix64 construction of diffudf_amd/synth.py, counter g): u1 = (b1 >> 11) 2^-53, r1
 *   and r2 alike; with `uniforms` (device, (n,3) double: u1, r1, r2 per sample, each in [0, 1)) those replace them.  The face is the
 *   first f with c_f > floor(u1 2^53 * W / 2^53) — `searchsorted(c, t, side="right")` —, the point ((1 - s) A + s (1 - r2) B) + s r2 C
 *   with s = sqrt(r1), in fp64 and in that order, rounded to fp32.  out_points (n,3); out_normals (n,3, or NULL) the face's fp32
 *   normal; out_face (n, or NULL) int64.  A row of `uniforms` outside [0, 1) gives a NaN point and face -1.  The result is a pure
 *   function of (mesh, seed, g): samples [0, a + b) are samples [0, a) followed by [a, a + b), bit for bit.
 *   The call reads one status word back on `stream` (it waits for the stream once; not for graph capture) and returns
 *   DUDF_E_BADCFG for F <= 0, V <= 0, n < 0, start < 0, a NULL input or a mesh whose every face has nn = 0; DUDF_E_BADMODE for a face
 *   index outside [0, V) (not dereferenced) or a non-finite nn; DUDF_E_UNSUPPORTED for F >= 2^31.  n == 0 still writes
 *   out_face_normals and out_area.  workspace: dudf_mesh_sample_surface_workspace(F) (0 for an F the call refuses), 256-byte aligned,
 *   else DUDF_E_WORKSPACE. */
size_t dudf_mesh_sample_surface_workspace(int64_t F);
int dudf_mesh_sample_surface(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int64_t start, int64_t n,
                             uint64_t seed, const double* uniforms, float* out_points, float* out_normals, int64_t* out_face,
                             float* out_face_normals, double* out_area, void* workspace, size_t workspace_bytes, void* stream);

/* dudf_distance_stats — of dist (n) fp32 (device), non-negative: out_counts (device, K + 1 int64) = the rows with (double)d <= tau_k
 *   (inclusive) for the K thresholds (HOST, K doubles), then the NaN rows; out_max (device, 1 fp32) = the maximum, taken on the bits;
 *   out_sums (device, 2 doubles) = sum d and sum d*d.  NaN rows enter the last count only; +inf is a value.  Counts and maximum do
 *   not depend on order; the sums are per-workgroup partials added in index order (as dudf_chamfer_terms): a repeated call is
 *   bit-identical.  n == 0: zero counts, maximum 0, zero sums.  K < 0 or K > 16: DUDF_E_UNSUPPORTED; n < 0 or a NULL pointer:
 *   DUDF_E_BADCFG.  workspace: dudf_distance_stats_workspace_bytes(n). */
size_t dudf_distance_stats_workspace_bytes(int64_t n);
int dudf_distance_stats(const float* dist, int64_t n, const double* thresholds, int K, int64_t* out_counts, float* out_max,
                        double* out_sums, void* workspace, size_t workspace_bytes, void* stream);

/* K nearest neighbours and consistent normal orientation — the device side of pytorch3d's `knn_points(x, y, K=K)` and of open3d's
 * `orient_normals_consistent_tangent_plane(k)` (reference generate_pc.py:40).  csrc/dudf_orient.hip; the rules are DESIGN.md §3.7
 * (tests/orient_oracle.py restates them in numpy).  These entry points arrived after ABI 8 without changing any existing signature.
 *
 * dudf_knn_points — for every row of x (n,3) the K rows of y (m,3) at the smallest SQUARED Euclidean distance, both fp32: out_dist
 *   (n,K) fp32 and out_idx (n,K) int64, either may be NULL, each row ascending by (distance bits, index).  A pair's distance is the
 *   expression of dudf_nearest_points (norm 2), so K = 1 repeats that call bit for bit on finite inputs.  exclude_self != 0 (meant for
 *   x == y): row i never returns index i.  A row with fewer than K candidates is padded with +inf / -1.  Rows of y with a NaN or an
 *   infinity, and pairs whose distance overflows, are never returned; such a row of x gets NaN distances and -1 indices.
 *   mode 0: a uniform cell list over y, built on the device by this call inside the workspace, walked in growing shells (the default
 *   of the Python side); mode 1: the tiled scan over all of y.  Both return the same bits on every input, ties included.  The result
 *   is a function of the inputs alone: not of launch geometry, not of the order in which atomics arrive; two calls are bit-identical.
 *   mode not in {0, 1}: DUDF_E_BADMODE; n < 0: DUDF_E_BADCFG; n or m >= 2^31, K < 1 or K > 16: DUDF_E_UNSUPPORTED; n == 0: nothing is
 *   launched, 0; m <= 0 or a NULL x / y with n > 0: DUDF_E_BADCFG; workspace: dudf_knn_workspace_bytes(n, m, K, mode) (0 for arguments
 *   the call refuses), 256-byte aligned, else DUDF_E_WORKSPACE.  Every check is made before the first device call.
 * dudf_knn_grid_build — the cell list of mode 0 alone, into a workspace of dudf_knn_workspace_bytes(0, m, 1, 0) or more (what
 *   dudf_knn_points does first; here for timing).  m >= 2^31: DUDF_E_UNSUPPORTED; m <= 0 or y NULL: DUDF_E_BADCFG. */
size_t dudf_knn_workspace_bytes(int64_t n, int64_t m, int K, int mode);
int dudf_knn_grid_build(const float* y, int64_t m, void* workspace, size_t workspace_bytes, void* stream);
int dudf_knn_points(const float* x, int64_t n, const float* y, int64_t m, int K, int exclude_self, int mode, float* out_dist,
                    int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* dudf_orient_normals — signs for the normals (n,3) fp32 of the cloud points (n,3) fp32 such that neighbours agree: the minimum
 *   spanning forest of the graph with one edge per slot of knn_idx (n,K) int64 (as dudf_knn_points wrote it; a slot outside [0, n) or
 *   equal to its own row is no edge and is not dereferenced), weight 1 - |n_i . n_j| in fp32, ties broken by the slot number; an edge
 *   with n_i . n_j < 0 flips.  Per connected component the vertex with the largest z (smallest index among equal z) ends with n_z >= 0.
 *   out_normals (n,3) fp32 = the input or its exact negation (may be `normals` itself); out_flip (n) uint8; out_component (n) int64 =
 *   the smallest vertex index of the component; out_counts (device, 2 int64) = components, forest edges.  Any output may be NULL.
 *   host_stats (HOST memory, 2 int64, may be NULL) = Borůvka rounds and kernel launches of this call.  Integer atomics only: two calls
 *   are byte-identical.  The call synchronises the stream once per round (at most ceil(log2 n) + 1 rounds).
 *   n < 0: DUDF_E_BADCFG; n >= 2^31, K < 1, K > 16 or n * K >= 2^32: DUDF_E_UNSUPPORTED; n == 0: nothing is launched, 0; a NULL input
 *   with n > 0: DUDF_E_BADCFG; workspace: dudf_orient_workspace_bytes(n, K) (0 for arguments the call refuses), else DUDF_E_WORKSPACE. */
size_t dudf_orient_workspace_bytes(int64_t n, int K);
int dudf_orient_normals(const float* points, const float* normals, const int64_t* knn_idx, int64_t n, int K, float* out_normals,
                        unsigned char* out_flip, int64_t* out_component, int64_t* out_counts, int64_t* host_stats, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Raw scans: normals estimated from the k-NN graph and the statistical outlier test — the device side of open3d's
 * `estimate_normals(KDTreeSearchParamKNN(k))` and `remove_statistical_outlier(nb_neighbors, std_ratio)`, which a cloud without normals
 * needs before dudf_orient_normals.  csrc/dudf_cloudprep.hip; the rules are DESIGN.md §3.8 (tests/cloudprep_oracle.py restates them in
 * numpy).  These entry points arrived after ABI 8 without changing any existing signature.
 *
 * dudf_estimate_normals — per point the eigenvector of the smallest eigenvalue of its neighbourhood's covariance.  points (n,3) fp32,
 *   knn_idx (n,K) int64 as dudf_knn_points wrote it.  The neighbourhood of row i is i itself when include_self != 0, then the slots of
 *   row i in slot order; a slot outside [0, n) or equal to i is skipped and never dereferenced; c is the neighbourhood size.  The mean
 *   is formed in fp64 (the sum starts at 0.0 and runs in neighbourhood order, then is divided by c), the covariance is the sum of the
 *   outer products of (p_j - mean) in fp64 in the same order, without contraction, divided by c (lower triangle).  The cyclic Jacobi
 *   solver of the loss kernels gives ascending eigenvalues; the normal is the first eigenvector, normalised in fp64 and rounded once
 *   to fp32, with the sign the solver gives (orientation is dudf_orient_normals' job).  c < 3, an all-zero covariance (coincident
 *   points) or a non-finite coordinate in the neighbourhood: normal (0, 0, 1), eigenvalues 0 (open3d's fallback).
 *   out_normals (n,3) fp32; out_eigenvalues (n,3) fp64 and out_count (n) int32 = c may be NULL.  Two calls are byte-identical.
 *   n < 0: DUDF_E_BADCFG; K < 1, K > 16 or n >= 2^31: DUDF_E_UNSUPPORTED; n == 0: nothing is launched, 0; points, knn_idx or
 *   out_normals NULL with n > 0: DUDF_E_BADCFG; workspace: dudf_estimate_normals_workspace_bytes(n, K) (0 for arguments the call
 *   refuses; the cloud as 16-byte rows), 256-byte aligned, else DUDF_E_WORKSPACE.  Every check is made before the first device call. */
size_t dudf_estimate_normals_workspace_bytes(int64_t n, int K);
int dudf_estimate_normals(const float* points, const int64_t* knn_idx, int64_t n, int K, int include_self, float* out_normals,
                          double* out_eigenvalues, int* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* dudf_cloud_outliers — the statistical outlier test on knn_dist (n,K) fp32, the SQUARED distances dudf_knn_points wrote.
 *   out_mean_dist (n) fp64: d_i = the mean over the finite slots of row i of sqrt((double)dist), summed in slot order; a row with no
 *   finite slot gets +inf, is dropped and stays out of the statistics.  out_stats (device, 3 doubles, may be NULL) = mu, sigma,
 *   threshold: the population mean and standard deviation of the finite d_i in fp64 — per-workgroup partials added in index order by
 *   one workgroup, sigma from the centred second pass — and mu + std_ratio * sigma.  out_keep (n) uint8 = d_i <= threshold;
 *   out_kept_idx (n int64, may be NULL) = the kept rows in ascending order, out_counts (device, 1 int64, may be NULL) = how many: the
 *   library reads nothing back.  No atomics: two calls are byte-identical.  No finite row: the statistics are NaN and nothing is kept.
 *   Refusals as dudf_estimate_normals (NULL knn_dist, out_mean_dist or out_keep with n > 0: DUDF_E_BADCFG); workspace:
 *   dudf_cloud_outliers_workspace_bytes(n, K). */
size_t dudf_cloud_outliers_workspace_bytes(int64_t n, int K);
int dudf_cloud_outliers(const float* knn_dist, int64_t n, int K, double std_ratio, double* out_mean_dist, unsigned char* out_keep,
                        double* out_stats, int64_t* out_kept_idx, int64_t* out_counts, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Exact unsigned distance from points to a triangle mesh with a bounding-volume hierarchy — the device side of open3d's
 * `RaycastingScene.add_triangles / compute_distance` (reference generate_df.py:108-110).  csrc/dudf_bvh.hip (the index), csrc/dudf_meshdist.hip (the queries).  Like the Chamfer
 * entry points these arrived after ABI 8 without changing any existing signature.  tri (n_tri,9) fp32 is the triangle soup
 * dudf_sample_batch takes; 0 < n_tri < 2^31 (n_tri <= 0: DUDF_E_BADCFG, larger: DUDF_E_UNSUPPORTED).
 *
 * dudf_mesh_index_bytes — size of the index of n_tri triangles (O(n_tri): sorted copy of the soup, original indices, the boxes of a
 *   complete binary tree over leaves of 8 triangles); 0 for an n_tri out of range.  The buffer is 256-byte aligned device memory
 *   (else DUDF_E_WORKSPACE).
 * dudf_mesh_morton_codes — codes (n_tri) int64 = 63-bit Morton code of every triangle's centroid inside the bounding box of all
 *   vertices.  The caller sorts them — a STABLE sort, so that the index is a function of the triangles alone — and passes the
 *   permutation on.  Uses the head of `index` as scratch.
 * dudf_mesh_index_build — builds the index for `order` (n_tri) int64, order[s] = original index of the s-th triangle along the
 *   curve; any permutation gives a correct index, the Morton order gives a fast one.  Nothing comes back to the host; the 32-bit
 *   word at byte DUDF_MESH_INDEX_FLAGS_OFFSET of the index then holds DUDF_MESH_FLAG_NONFINITE if a vertex is NaN or infinite and
 *   DUDF_MESH_FLAG_BAD_ORDER if an entry of `order` lies outside [0, n_tri) (it is not dereferenced); an index with a flag set
 *   must not be queried.  Two builds from the same inputs are byte-identical.
 * dudf_mesh_distance — for pts (n_pts,3) fp32, every output optional (NULL): out_dist (n_pts) fp32 = sqrt of the minimum over all
 *   triangles of the fp64 squared distance (the arithmetic of dudf_sample_batch), rounded once; out_tri (n_pts) int64 = the
 *   triangle that attains it, in the caller's order, the smallest index among equal distances; out_closest (n_pts,3) fp32 = the
 *   closest point on that triangle; *out_stats (device int64, ADDED to) = exact triangle evaluations of the call.
 *   index == NULL: brute force over all triangles — the cross-check; with an index the same bits (a subtree is skipped only on a
 *   safe-side bound STRICTLY above the best exact value).  A point with a NaN coordinate: distance NaN, triangle -1, closest NaN.
 *   n_pts == 0: nothing is launched, 0.
 * dudf_mesh_occupancy — `scene.compute_occupancy(points)` (behind `compute_signed_distance`, reference src/dataset.py:35,50,
 *   src/render_st.py:275-276) by ray parity: out_count (n_pts) int32 = how many triangles the ray from the point along +x crosses,
 *   out_inside (n_pts) bytes = count & 1; either may be NULL.  The ray is axis-aligned, so a crossing is a point-in-triangle test of
 *   (p.y, p.z) in the triangle's (y, z) projection plus one comparison in x, all on the fp32 inputs: (p.y, p.z) must lie in the
 *   triangle's closed (y, z) extent with max x >= p.x; a triangle of zero projected area counts 0; each edge function is evaluated
 *   in fp64 from the edge's lower vertex to its higher one (lexicographic on (y, z, x)) and negated for the triangle that runs the
 *   edge the other way, so two triangles sharing an edge see exactly opposite values; a zero lies on the left of the edge taken
 *   from its lower to its higher vertex (a footprint is open at its low-y and high-z borders, closed at its high-y and low-z ones);
 *   the three sides must agree and the crossing's x, interpolated in fp64, must be > p.x.  index == NULL scans every triangle;
 *   with an index the same counts (a box is visited iff (p.y, p.z) is in its closed (y, z) extent and its hi.x >= p.x: compares
 *   of stored floats).  A point with a NaN coordinate: count -1, inside 0.  n_pts == 0: nothing is launched, 0.
 * dudf_mesh_trace_rays — the marching loop of `create_projectional_image_gt` (reference src/render_st.py:255-268) in one launch, one
 *   lane per ray: rays (n_rays,3) double; t0 (n_rays,3) double and mask (n_rays) bytes are updated in place; hits (n_rays) bytes is
 *   written.  Per iteration of a ray whose mask is set: d = the fp32 distance dudf_mesh_distance gives for float32(t0) (same walk,
 *   same arithmetic, same bits); t0 += ray * (double)d, product and sum rounded separately; d < float32(surface_eps) (numpy's
 *   comparison of float32 distances with a Python float): hit, mask cleared; otherwise the mask is cleared once a coordinate of t0
 *   is not inside (-bound, bound) (the reference: 1.3).  A NaN position never hits and clears the mask.  index == NULL: the same with
 *   the brute-force scan.  max_iterations < 0: DUDF_E_BADCFG; n_rays == 0: nothing is launched, 0. */
#define DUDF_MESH_INDEX_FLAGS_OFFSET 24
#define DUDF_MESH_FLAG_NONFINITE 1
#define DUDF_MESH_FLAG_BAD_ORDER 2
size_t dudf_mesh_index_bytes(int64_t n_tri);
int dudf_mesh_morton_codes(const float* tri, int64_t n_tri, void* index, size_t index_bytes, int64_t* codes, void* stream);
int dudf_mesh_index_build(const float* tri, int64_t n_tri, const int64_t* order, void* index, size_t index_bytes, void* stream);
int dudf_mesh_distance(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const float* pts, int64_t n_pts,
                       float* out_dist, int64_t* out_tri, float* out_closest, int64_t* out_stats, void* stream);
int dudf_mesh_occupancy(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const float* pts, int64_t n_pts,
                        int32_t* out_count, unsigned char* out_inside, void* stream);
int dudf_mesh_trace_rays(const float* tri, int64_t n_tri, const void* index, size_t index_bytes, const double* rays, double* t0,
                         unsigned char* mask, unsigned char* hits, int64_t n_rays, double surface_eps, int max_iterations,
                         double bound, void* stream);

/* The field part of `extract_fields` (reference src/render_mc.py:20-99) for grid points start .. start+count-1 of the
 * regular grid_n^3 grid on [-1,1]^3 (linear index, first axis slowest, coordinates derived from the index):
 * out_df (count) = inverse(gt_mode, |f|, alpha) with inverse_mode 0 'tanh' / 1 'siren' / 2 'squared'
 * (src/inverses.py:3-21); out_vec (count,3) = -normalize(df/dx); *out_flag_count (device int) = number of points whose
 * normalised gradient is shorter than 0.04 — the only ones for which the reference substitutes the sign-aligned top
 * Hessian eigenvector (:80-93); the caller re-queries those with dudf_query_frame.  12 B in, 16 B out per point. */
int dudf_grid_fields(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int64_t start, int64_t count,
                     int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count,
                     void* workspace, size_t workspace_bytes, void* stream);

/* CAP-UDF cell extraction — replaces the per-cell Python loop of `extract_mesh_CAP(ndf, grad, resolution)` (reference
 * src/render_mc.py:201-256) on the fields dudf_grid_fields produced, which stay on the device:
 *   ndf (grid_n^3) float, grad (grid_n^3, 3) float, first grid axis slowest;  threshold = 0.008 in the reference (:205).
 * A cell is emitted when min(ndf over its 8 corners) <= threshold and, with every corner signed by
 * dot(grad[corner 000], grad[corner]) < 0 (:224), some corner is negative (:230); it then contributes the vertices and
 * triangles of marching cubes at iso 0 on its 2x2x2 values, shifted by its index and mapped to [-1,1]^3 (:236-252), in
 * the reference's (i, j, k) loop order.  The per-cell marching cubes replaces `mcubes.marching_cubes` (PyMCubes,
 * third-party, absent here; conventions and table: oracle/capudf_oracle.py, tools/gen_mc_table.py).
 * Two calls because the output size is data dependent:
 *   dudf_capudf_count -> out_counts (device, 3 x int64): emitted cells, vertices, triangles;
 *   dudf_capudf_emit  -> out_vertices (V,3) double, out_triangles (T,3) int64 (indices into out_vertices),
 *                        out_cells (C,3) int64 or NULL; same ndf / grad / threshold / workspace as the count call.
 * workspace: dudf_capudf_workspace_bytes(grid_n), 256-byte aligned, else DUDF_E_WORKSPACE. */
size_t dudf_capudf_workspace_bytes(int64_t grid_n);
int dudf_capudf_count(const float* ndf, const float* grad, int64_t grid_n, double threshold, int64_t* out_counts,
                      void* workspace, size_t workspace_bytes, void* stream);
int dudf_capudf_emit(const float* ndf, const float* grad, int64_t grid_n, double threshold, double* out_vertices,
                     int64_t* out_triangles, int64_t* out_cells, void* workspace, size_t workspace_bytes, void* stream);

/* The same extraction on a brick-sparse narrow band, for grids whose N^3 fields are out of reach.  The dense calls
 * above are the exact ones; these evaluate the network only where the selection rule below allows an active cell.
 *   grid_n = N >= 2 points per side, m = N - 1 cells, brick edge B = `brick` in {4, 8}.  Brick (b0, b1, b2) owns the grid points
 *   [b_d B, b_d B + B) per axis; the storage lattice has nl = m / B + 1 bricks per side, brick id = (b0 nl + b1) nl + b2; the cell
 *   bricks are those with every b_d < nb = ceil(m / B).  Storage: df [slot][B][B][B] float, vec [slot][B][B][B][3] float, slot
 *   [nl^3] int32 = the slot of a stored brick or -1, slots in ascending brick id.  Coordinates are formed from the index as
 *   dudf_grid_fields forms them, so a stored point has the dense grid's coordinates bit for bit; points of a partial brick beyond
 *   index m are evaluated at the clamped index and never read.
 * dudf_grid_fields_lattice: points start .. start+count-1 of the coarse lattice of (nb + 1)^3 points (first axis slowest) at fine
 *   indices min(c_d B, m); out_df, out_vec, out_flag_count as dudf_grid_fields; out_vec NULL: value only, no reverse sweep, no flag
 *   count.  Workspace of dudf_workspace_bytes_query with (cfg, count, 0).
 * dudf_sparse_select: coarse_df = that lattice.  A cell brick is a CANDIDATE when the minimum over its 8 lattice corners, compared
 *   as double, is <= bound, or a corner is NaN; a brick is STORED when it is a candidate b or a brick b + delta, delta in {0,1}^3,
 *   of a candidate inside the lattice: every corner of every cell of a candidate brick is then stored exactly once.  The caller
 *   forms bound = threshold + L (sqrt(3) / 2) B (2 / (N - 1)) in double for an L-Lipschitz df.  Outputs (device): out_slot [nl^3],
 *   out_stored_ids and out_candidate_ids (ascending brick ids, room for nl^3 int32 each), out_counts 2 x int64 = stored, candidate
 *   bricks.  No atomics: the result is the same on every run.  Workspace: dudf_sparse_select_bytes with (grid_n, brick).
 * dudf_grid_fields_bricks: df and vec of the B^3 points of each of the n_bricks bricks listed at brick_ids (a range of the stored
 *   list), through the sweeps and epilogue of dudf_grid_fields; out_df / out_vec point at the first of these bricks' slots (a range of
 *   slots is contiguous).  Workspace of dudf_workspace_bytes_query with (cfg, n_bricks B^3, 0).
 * dudf_capudf_sparse_count / _emit: dudf_capudf_count / _emit over the cells of the n_candidates candidate bricks, one thread per
 *   cell, a cell's 8 corners addressed through `slot` — the active test, sign rule, table, interpolation and vertex formula (with the
 *   GLOBAL cell index) are the dense kernels' own code.  Cells beyond m in a partial brick are skipped; a corner in a brick that is
 *   not stored reads as NaN (the cell is skipped).  Emission order: candidate bricks ascending, cells in local (i, j, k) order.
 *   Outputs as the dense calls; out_cells holds global cell indices.  Workspace: dudf_capudf_sparse_workspace_bytes with (grid_n, brick,
 *   n_candidates).
 * Refusals, all before the first device call: brick not in {4, 8}, grid_n < 2, a NULL required pointer, a range outside the lattice:
 *   DUDF_E_BADCFG; a bad inverse_mode: DUDF_E_BADMODE; more than 2^31 - 1 lattice entries or points in one call: DUDF_E_UNSUPPORTED
 *   — the coarse lattice sets the largest grid: (nb + 1)^3 <= 2^31 - 1, that is N <= 10313 with B = 8 and N <= 5157 with B = 4. */
int dudf_grid_fields_lattice(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int brick, int64_t start, int64_t count,
                             int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count, void* workspace,
                             size_t workspace_bytes, void* stream);
size_t dudf_sparse_select_bytes(int64_t grid_n, int brick);
int dudf_sparse_select(const float* coarse_df, int64_t grid_n, int brick, double bound, int32_t* out_slot, int32_t* out_stored_ids,
                       int32_t* out_candidate_ids, int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
int dudf_grid_fields_bricks(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int brick, const int32_t* brick_ids,
                            int64_t n_bricks, int inverse_mode, double alpha, float* out_df, float* out_vec, int* out_flag_count,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t dudf_capudf_sparse_workspace_bytes(int64_t grid_n, int brick, int64_t n_candidates);
int dudf_capudf_sparse_count(const float* df, const float* vec, const int32_t* slot, const int32_t* candidate_ids,
                             int64_t n_candidates, int64_t grid_n, int brick, double threshold, int64_t* out_counts,
                             void* workspace, size_t workspace_bytes, void* stream);
int dudf_capudf_sparse_emit(const float* df, const float* vec, const int32_t* slot, const int32_t* candidate_ids,
                            int64_t n_candidates, int64_t grid_n, int brick, double threshold, double* out_vertices,
                            int64_t* out_triangles, int64_t* out_cells, void* workspace, size_t workspace_bytes, void* stream);

/* The raw network output on the grid — the value loop of `get_mesh_sdf` (reference src/render_mc.py:335-348) for grid points
 * start .. start+count-1 of the regular grid_n^3 grid on [-1,1]^3 (indexing and coordinates as dudf_grid_fields): out_f (count) = f,
 * sign kept — no |.|, no inverse map, no gradient (the forward sweep only).  Workspace of dudf_workspace_bytes_query(cfg, count, 0). */
int dudf_grid_values(const dudf_net_cfg* cfg, const float* theta, int64_t grid_n, int64_t start, int64_t count, float* out_f,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Lewiner marching cubes of a signed volume on the device — what `marching_cubes(volume, level)` does for `get_mesh_sdf` (reference
 * src/render_mc.py:389, scikit-image on the host there) without the volume leaving the device.  volume [nz][ny][nx] float (device,
 * first axis slowest), corner value (double)volume - level, inside where > 0, every cube in raster order.  The Lewiner tables are an
 * input as they are for libdudf_meshudf.so (include/dudf_meshudf.h; order and packing of `marching_cubes._pack_luts`): lut_data int8
 * on the DEVICE (4-byte aligned, at most 18 KiB), lut_offsets[n_luts] and lut_dims[n_luts][3] on the HOST, n_luts = 51.
 * The output equals dudf_mc_lewiner_run of that library bit for bit and in the same order.  Two calls, the size being data dependent:
 *   dudf_mc_lewiner_count -> out_counts (device, 2 x int64): vertices V, triangles T;
 *   dudf_mc_lewiner_emit  -> out_vertices (V,3) float (x, y, z in grid units), out_faces (T,3) int32, out_normals (V,3) float (the
 *                            unnormalised sums), out_values (V) float; same volume / level / tables / workspace as the count call.
 * Dimensions 2 .. 2048 each; V must stay below 2^31 (int32 faces, as the reference).  workspace: dudf_mc_lewiner_workspace_bytes(nz, ny,
 * nx), 256-byte aligned, else DUDF_E_WORKSPACE. */
size_t dudf_mc_lewiner_workspace_bytes(int64_t nz, int64_t ny, int64_t nx);
int dudf_mc_lewiner_count(const float* volume, int64_t nz, int64_t ny, int64_t nx, double level, const signed char* lut_data,
                          const int64_t* lut_offsets, const int32_t* lut_dims, int n_luts, int64_t* out_counts, void* workspace,
                          size_t workspace_bytes, void* stream);
int dudf_mc_lewiner_emit(const float* volume, int64_t nz, int64_t ny, int64_t nx, double level, const signed char* lut_data,
                         const int64_t* lut_offsets, const int32_t* lut_dims, int n_luts, float* out_vertices, int32_t* out_faces,
                         float* out_normals, float* out_values, void* workspace, size_t workspace_bytes, void* stream);

/* Mesh clean-up on the device — what `extract_mesh_MESHUDF` asks of trimesh (reference src/render_mc.py:136-197: process, duplicate and
 * degenerate faces, fill_holes, border smoothing).  vertices (V,3) double, faces (F,3) int64, both on the device; V, F < 2^31
 * (DUDF_E_UNSUPPORTED beyond); workspaces 256-byte aligned.  The rules are DESIGN.md §3 "Mesh clean-up" (tests/meshclean_oracle.py restates
 * them; the device result equals it bit for bit and is the same from run to run).  One ROUND:
 *   1. a face with an index outside [0, V) or a non-finite vertex coordinate is dropped (counted, never dereferenced);
 *   2. vertices used by the remaining faces weld on the key rint(v * 10^digits) per coordinate (int64, 0 <= digits <= 15) into the
 *      smallest original index of the key, which keeps its own coordinates;
 *   3. faces are remapped, then pruned: degenerate (longest edge L <= 1e-8 or |(v1-v0) x (v2-v0)| / L <= 1e-8, compared squared), then
 *      all but the smallest face index of every vertex set;
 *   4. unused vertices go; survivors keep their relative order.
 * fill_holes = 1 adds, behind the surviving faces and in ascending smallest vertex, the faces that close the border cycles of 3 or 4
 * vertices which lie on exactly two border edges each (one face / two faces, wound against the existing face on the cycle's edge).
 *   dudf_mesh_clean_count -> out_counts (device, 9 x int64): V', F', welded vertices, unreferenced vertices, duplicate faces, degenerate
 *                            faces, 3-edge holes, 4-edge holes, invalid faces; maps and flags stay in the workspace;
 *   dudf_mesh_clean_emit  -> out_vertices (V',3) double, out_faces (F',3) int64; same arguments and workspace as the count call (a
 *                            workspace that does not hold that call's result is left alone: nothing is written). */
size_t dudf_mesh_clean_workspace_bytes(int64_t V, int64_t F);
int dudf_mesh_clean_count(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int digits, int fill_holes,
                          int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
int dudf_mesh_clean_emit(const double* vertices, int64_t V, const int64_t* faces, int64_t F, int digits, int fill_holes,
                         double* out_vertices, int64_t* out_faces, void* workspace, size_t workspace_bytes, void* stream);

/* Border edges — undirected edges (u < w, u != w) that exactly one face uses; faces with an index outside [0, V) are skipped — and the
 * reference's border smoothing (src/render_mc.py:169-197).  F < 2^32 / 6.
 *   dudf_mesh_border_count -> out_count (device, 1 x int64): E;    dudf_mesh_border_edges -> out_edges (E,2) int64, ascending; same
 *                             faces and workspace as the count call;
 *   dudf_mesh_smooth_borders: `iterations` Jacobi steps v += lambda * (mean(border neighbours) - v) on the endpoints of the border
 *                             edges, in double, the sum starting at 0.0 and taking the neighbours in ascending index order, every
 *                             average formed from the positions before the step. */
size_t dudf_mesh_border_workspace_bytes(int64_t V, int64_t F);
int dudf_mesh_border_count(int64_t V, const int64_t* faces, int64_t F, int64_t* out_count, void* workspace, size_t workspace_bytes,
                           void* stream);
int dudf_mesh_border_edges(int64_t V, const int64_t* faces, int64_t F, int64_t* out_edges, void* workspace, size_t workspace_bytes,
                           void* stream);
int dudf_mesh_smooth_borders(double* vertices_inout, int64_t V, const int64_t* faces, int64_t F, int iterations, double lambda,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Mesh topology on the device — consistent winding, connected components and their sizes: what the reference's users ask of trimesh's
 * `fix_winding` / `split`.  csrc/dudf_meshtopo.hip; the rules are DESIGN.md §3.6b (tests/meshtopo_oracle.py restates them; the device
 * result equals it exactly and is the same from run to run).  faces (F,3) int64, vertices (V,3) double or NULL, on the device;
 * 0 <= V < 2^31, 6 F < 2^32 (DUDF_E_UNSUPPORTED beyond, before any device call); F = 0 is valid.
 *   - a face with an index outside [0, V) or two equal indices is IGNORED: never dereferenced, no edge, its own component, flip 0;
 *   - every other face uses its three directed edges under the undirected key (min << 32) | max.  One use: a BORDER edge.  Two uses:
 *     a MANIFOLD edge, which links its two faces with the sign s = 1 iff both traverse it in the same direction.  More: NON-MANIFOLD,
 *     counted, links nothing;
 *   - the minimum spanning forest of the face graph under the key (every key is one link: the forest is unique) carries the flip
 *     parity; a face's component label is the smallest face index of its component, that face keeps its winding and every other
 *     face's flip is its parity relative to it.  A flipped face (a, b, c) is written (a, c, b);
 *   - INCONSISTENT edges are the manifold edges both faces still traverse the same way after the flips (a non-orientable component).
 * Outputs (device): out_faces (F,3) int64 (may not alias faces), out_component (F,) int64, out_flip (F,) uint8, out_component_faces
 * (F,) int64 and out_component_area_q (F,) uint64 (non-zero at label positions only), out_counts 8 x int64: components (ignored faces
 * included), forest edges, manifold, border, non-manifold edges, ignored faces, flipped faces, inconsistent edges.  With vertices the
 * area of a component is sum(q) * 2^-31, q = (uint64) rint(min(nn, 16) * 2^30) per face and nn = sqrt((n0 n0 + n1 n1) + n2 n2) of
 * n = (b - a) x (c - a) as in dudf_mesh_sample_surface (a non-finite nn: q = 0); integer sums, the same in any order.  Without: zeros.
 * One small read-back per Borůvka round (at most ceil(log2 F) + 1 rounds). */
size_t dudf_mesh_topology_workspace_bytes(int64_t F);
int dudf_mesh_topology(const int64_t* faces, int64_t F, int64_t V, const double* vertices, int64_t* out_faces, int64_t* out_component,
                       unsigned char* out_flip, int64_t* out_component_faces, uint64_t* out_component_area_q, int64_t* out_counts,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Submesh by face mask: the faces with keep[f] != 0 in their order (a kept face with an index outside [0, V) counts as not kept), the
 * vertices they use in their relative order, faces re-indexed.  keep (F,) uint8.  V, F < 2^31.
 *   dudf_mesh_submesh_count -> out_counts (device, 2 x int64): V', F'; the maps stay in the workspace;
 *   dudf_mesh_submesh_emit  -> out_vertices (V',3) double, out_faces (F',3) int64; same arguments and workspace as the count call (a
 *                              workspace that does not hold that call's result is left alone: nothing is written). */
size_t dudf_mesh_submesh_workspace_bytes(int64_t V, int64_t F);
int dudf_mesh_submesh_count(int64_t V, const int64_t* faces, int64_t F, const unsigned char* keep, int64_t* out_counts, void* workspace,
                            size_t workspace_bytes, void* stream);
int dudf_mesh_submesh_emit(const double* vertices, int64_t V, const int64_t* faces, int64_t F, const unsigned char* keep,
                           double* out_vertices, int64_t* out_faces, void* workspace, size_t workspace_bytes, void* stream);

/* Mesh simplification: quadric vertex clustering on a uniform lattice (Lindstrom's one-pass simplification) with border quadrics.
 * vertices (V,3) double, faces (F,3) int64, origin: 3 doubles ON THE HOST, cell: the lattice edge h.  The rules (DESIGN.md §3.6c,
 * restated by tests/simplify_oracle.py):
 *   - a face with an index outside [0, V) or a non-finite coordinate is INVALID: dropped, counted, never dereferenced; another face with
 *     a repeated index is dropped and counted with `collapsed`;
 *   - the cell of a vertex is c_d = floor((v_d - origin_d) * inv), inv = 1.0 / h, saturated to [0, 2^21 - 1]; its key is
 *     c_0 << 42 | c_1 << 21 | c_2.  Corner k of a valid face contributes a RECORD iff no corner j < k of the face has the same key;
 *     records are ordered by (key, face index); the occupied cells are the distinct keys, ascending;
 *   - a record adds, in the frame u = (p - o_c) * inv of its cell (o_c = origin + (c + 0.5) * h), the plane quadric of the unnormalised
 *     normal n = (u_1 - u_0) x (u_2 - u_0) (weight: area squared) and, with boundary_weight > 0, for k = 0, 1, 2 the quadric of the plane
 *     through edge k perpendicular to the face, times boundary_weight / (e.e), when edge k is used by exactly one valid face and one of
 *     its endpoints lies in the cell.  A cell's ten numbers are summed sequentially in record order, in fp64, by one thread; beside
 *     them the record count and xhat, the mean of each record's first corner in the cell;
 *   - placement: the eigen-decomposition of A; from xhat, the minimiser's components along the eigenvectors with lam_i > tau * max|lam|;
 *     xhat itself (FALLBACK, counted) if an eigenvalue is not finite, all are zero or the result leaves the cell (not every
 *     |x_d| <= 0.5).  Position ((c_d + 0.5) + x_d) * h + origin_d;
 *   - faces over cells: fewer than three distinct cells: `collapsed`; of the faces with one set of cells the smallest index survives
 *     (`duplicate`); survivors keep order and winding; cells no survivor uses drop out, the others keep ascending key order.
 * Three calls around one stable sort of int64 keys, which is the caller's (as the Morton order of dudf_mesh_index_build):
 *   dudf_mesh_simplify_keys  -> out_keys (device, 3 F int64): per face corner its cell key, or -1 (sorts first) for a corner without a
 *                               record; the edge table and the face states stay in the workspace;
 *   dudf_mesh_simplify_count -> out_counts (device, 8 x int64): V', F', occupied cells C, collapsed, duplicate, invalid faces, border
 *                               edges, fallback cells.  sorted_keys / order: out_keys sorted ascending (stable) and the index each came
 *                               from.  place = 0 skips the per-cell sums and placement (fallback is then -1, and emit writes nothing): the
 *                               face count alone, for a search over h;
 *   dudf_mesh_simplify_emit  -> out_vertices (V',3) double, out_faces (F',3) int64 and, all five or none, per occupied cell
 *                               out_quadrics (C,10), out_xhat (C,3), out_cell_keys (C,), out_records (C,) int64, out_fallback (C,)
 *                               uint8.  Same mesh and workspace as the count call (a workspace that does not hold that call's result is
 *                               left alone: nothing is written).
 * Limits: V < 2^31 and 3 F < 2^31, else DUDF_E_UNSUPPORTED (workspace_bytes: 0); cell and 1 / cell finite and positive, origin finite,
 * boundary_weight >= 0, 0 < tau < 1, required pointers non-NULL, else DUDF_E_BADCFG; all checked before the first device call. */
size_t dudf_mesh_simplify_workspace_bytes(int64_t V, int64_t F);
int dudf_mesh_simplify_keys(const double* vertices, int64_t V, const int64_t* faces, int64_t F, const double* origin, double cell,
                            int64_t* out_keys, void* workspace, size_t workspace_bytes, void* stream);
int dudf_mesh_simplify_count(const double* vertices, int64_t V, const int64_t* faces, int64_t F, const double* origin, double cell,
                             double boundary_weight, double tau, const int64_t* sorted_keys, const int64_t* order, int place,
                             int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
int dudf_mesh_simplify_emit(const double* vertices, int64_t V, const int64_t* faces, int64_t F, double* out_vertices, int64_t* out_faces,
                            double* out_quadrics, double* out_xhat, int64_t* out_cell_keys, int64_t* out_records,
                            unsigned char* out_fallback, void* workspace, size_t workspace_bytes, void* stream);

/* Forward half of loss_s1 / loss_siren (reference src/loss_functions.py:123-155, :82-104):
 * SIREN forward, df/dx, the four weighted loss terms.  out_terms (device, 4 floats) receives
 * THIS RANK's share  sum_local(term_i) * weight / n_global  in the reference's dict order
 * (s1: sdf_on_surf, sdf_off_surf, hessian_constraint, grad_constraint;
 *  siren: sdf_on_surf, sdf_off_surf, normal_constraint, grad_constraint).
 * weights: host, 4 doubles.  The activations needed by dudf_loss_backward stay in `workspace`.
 * n_hess: loss_s1 with weights[2] != 0 (hessian_constraint, reference :140-145: eigh of the Hessian, top
 * eigenvector against the normal, on-surface points only) — the caller orders the batch so that the on-surface
 * points (sdf == 0) are EXACTLY the first n_hess (the reference sampler already yields [on | far | near],
 * src/dataset.py:55-70); they take the Hessian path (4 columns each), the others the plain path.  0 otherwise.
 * A batch that breaks this (weights[2] != 0 and some point i with (i < n_hess) != (sdf[i] == 0)) gets NaN for the
 * hessian_constraint term and, from dudf_loss_backward, a NaN gradient: the term would otherwise silently cover the wrong points.
 * Workspace: dudf_workspace_bytes_hess(cfg, n_local, n_hess). */
int dudf_loss_forward(const dudf_net_cfg* cfg, int mode, const float* theta,
                      const float* x, const float* normals, const float* sdf,
                      int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights, double alpha,
                      float* out_terms, void* workspace, size_t workspace_bytes, void* stream);

/* loss_s2 (reference src/loss_functions.py:106-121) needs the mean/std of the on-surface
 * predictions over the GLOBAL batch, so its forward is split in two:
 *   dudf_s2_forward_stats: SIREN forward, writes (count, sum, sum of squares) of y over this
 *       rank's on-surface points to stats (device, 3 doubles) — all-reduce(sum) them across ranks;
 *   dudf_s2_terms: out_terms[0] = |mean|*w0, out_terms[1] = std_unbiased*w1 (device, 2 floats),
 *       from the (all-reduced) stats. */
int dudf_s2_forward_stats(const dudf_net_cfg* cfg, const float* theta, const float* x, const float* sdf,
                          int64_t n_local, double* stats, void* workspace, size_t workspace_bytes,
                          void* stream);
int dudf_s2_terms(const double* stats, const double* weights, float* out_terms, void* stream);

/* Replaces `train_loss.backward()` (reference train.py:212-221) for the loss whose forward was
 * the last dudf_loss_forward / dudf_s2_forward_stats on this workspace.  cot (device, 4 floats;
 * 2 used for s2) = upstream gradient of each returned term (all ones in the reference loop).
 * dtheta (theta-sized, device) is overwritten when accumulate == 0, added to otherwise.
 * stats: device, 3 doubles (s2 only, else NULL). */
int dudf_loss_backward(const dudf_net_cfg* cfg, int mode, const float* theta,
                       const float* x, const float* normals, const float* sdf,
                       int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights, double alpha,
                       const float* cot, const double* stats, float* dtheta, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same backward in two steps, for overlapping the gradient all-reduce with the weight-gradient GEMM (one RCCL
 * all-reduce per layer group while the next group is still being computed; reference: `train_loss.backward()` hands
 * DistributedDataParallel its buckets in the same way):
 *   dudf_loss_backward_sweeps: loss cotangents + the two adjoint sweeps (everything of dudf_loss_backward except dW, db);
 *   dudf_weight_gradient: dW, db of the layers [layer_begin, layer_end) in theta order — 0 = first layer (3 -> H),
 *       1 .. L-1 = the hidden matrices, L = output layer; the slices of dtheta those layers own are overwritten
 *       (accumulate == 0) or added to.  The two thin layers (0 and L) are computed by ONE kernel (one pass over the
 *       columns): layer_begin = -1 asks for exactly those two (layer_end ignored); a range that contains only one of them
 *       must not be used with accumulate == 0 (the other one's slice would be added to without being zeroed).
 *       have_gradient_terms = 0 for loss_s2, 1 otherwise. */
int dudf_loss_backward_sweeps(const dudf_net_cfg* cfg, int mode, const float* theta, const float* normals, const float* sdf,
                              int64_t n_local, int64_t n_global, int64_t n_hess, const double* weights, double alpha,
                              const float* cot, const double* stats, void* workspace, size_t workspace_bytes, void* stream);
int dudf_weight_gradient(const dudf_net_cfg* cfg, int64_t n_local, int64_t n_hess, int have_gradient_terms, int layer_begin,
                         int layer_end, float* dtheta, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Generic differentiable fields, for losses written by the caller on top of (f, df/dx) instead of the
 * reference's three: dudf_fields_forward = dudf_query with the training stash kept in `workspace`;
 * dudf_fields_backward = d(sum_p ybar[p]*f[p] + gbar[p].df/dx[p]) / d(theta), i.e. what autograd's
 * backward through `model(x)` and `gradient(y, x)` (reference src/diff_operators.py:208-212 with
 * create_graph=True) delivers to the parameters.  ybar (n), gbar (n,3) or NULL. */
int dudf_fields_forward(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
                        float* out_f, float* out_g, void* workspace, size_t workspace_bytes, void* stream);
int dudf_fields_backward(const dudf_net_cfg* cfg, const float* theta, const float* x, int64_t n,
                         const float* ybar, const float* gbar, float* dtheta, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);

/* torch.optim.Adam.step() with default betas/eps semantics (reference train.py:334-337, :222) on
 * flat buffers.  step = 1-based count after this update.  grad_scale multiplies the gradient
 * first (1/world_size after an all-reduce(sum) is NOT needed here: ranks hold shares of one mean). */
int dudf_adam_step(float* theta, const float* dtheta, float* exp_avg, float* exp_avg_sq, int64_t n,
                   double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                   void* stream);

/* The same update with its step-dependent scalars read from DEVICE memory when the kernel runs, so that a training step
 * captured once in a HIP graph (hipStreamBeginCapture on `stream`; the reference's loop train.py:195-224 relaunches ~40
 * kernels from Python every step) replays with a new step count and learning rate each time:
 *   dudf_adam_schedule  (host only, no GPU work) fills rows (lr[i] / (1 - beta1^t), sqrt(1 - beta2^t)), t = first_step + i, of a
 *                       HOST table out (n_steps x 2 floats) — exactly the two values dudf_adam_step derives from (lr, step);
 *                       the caller uploads it;
 *   dudf_adam_step_scheduled  uses row *row of the DEVICE table sched (n_rows x 2 floats); row (device, one int64) is NOT advanced
 *                       by the call — the caller increments it on the same stream (inside the graph).  A row outside [0, n_rows)
 *                       writes NaN into theta: a replay past the end of the schedule must not train silently.
 * Bit-identical to dudf_adam_step(lr[i], step = first_step + i) (tests/test_graph_step_gpu.py). */
int dudf_adam_schedule(const double* lr, int64_t n_steps, int64_t first_step, double beta1, double beta2, float* out);
int dudf_adam_step_scheduled(float* theta, const float* dtheta, float* exp_avg, float* exp_avg_sq, int64_t n,
                             double beta1, double beta2, double eps, const float* sched, int64_t n_rows, const int64_t* row,
                             double grad_scale, void* stream);

/* Test/diagnostic hook: copy one stashed per-layer quantity of the last sweep into out (n,H) row-major.
 * which: 0 S (h|hdot), 1 C, 2 Q (q|qdot), 3 E, 4 A (A|Adot), 5 Z (zbar|zdotbar), 6 R (r | a|adot), 7 ZS (s|zdot);
 * layer: 0-based hidden layer; channel: 0 value, 1..3 tangent (Hessian-path points only). */
int dudf_debug_read_stash(const dudf_net_cfg* cfg, int which, int layer, int channel, int64_t n, int64_t n_hess,
                          float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Test/diagnostic hook: the symmetric 3x3 eigensolver of the loss kernels, the CAP-UDF eigen-frame, the curvature and the point-cloud
 * normals (csrc/dudf_eigh3.h: cyclic Jacobi in fp64) on k matrices of the caller's choosing, one thread per matrix.  H (k,3,3) fp64 row-major,
 * of which only the LOWER triangle is read (torch.linalg.eigh, reference src/loss_functions.py:142); out_lam (k,3) ascending;
 * out_V[m][i][j] = component i of v_j.  All three are device pointers.  Arrived after ABI 8 without changing any existing signature.
 *   k < 0: DUDF_E_BADCFG; k == 0: nothing is launched, 0; a NULL pointer with k > 0: DUDF_E_BADCFG. */
int dudf_debug_eigh3(const double* H, int64_t k, double* out_lam, double* out_V, void* stream);

/* Test/diagnostic hook: the loss stage of a training step on PLANTED fields — no sweep runs, so there is no theta.  The call
 *   1. scatters y (n), g (n,3) and the Hessians h (n_hess,3,3; h[p][i][k] = d2f/dx_i dx_k) of the first n_hess points into the per-column
 *      arrays of `workspace` the way a forward leaves them (the inverse of what dudf_fields_forward copies out; Hessian column k of
 *      point p is column 4p+1+k).  Padded columns and the y of the quads' tangent channels, which no loss kernel may read, hold NaN;
 *   2. zeroes the reduction scratch and fills the cotangent arrays with NaN;
 *   3. launches exactly what dudf_loss_forward + dudf_loss_backward launch between their sweeps: loss_s1 / loss_siren: the term
 *      kernel, then the cotangent kernel; loss_s2: the statistics, the two terms, then the cotangent kernel on `stats_in` (device, 3
 *      doubles: those of a larger global batch) or, when NULL, on the statistics just computed;
 *   4. gathers the cotangents per point: out_ybar (n), out_gbar (n,3), out_hbar (n_hess,3,3) with out_hbar[p][i][k] from column 4p+1+k.
 * out_terms (4 floats; loss_s2 writes two and leaves two zero), out_stats (3 doubles (count, sum, sum of squares); loss_s2 only),
 * out_pad_nonzero (1 int): the number of columns holding a float the stage owes a zero that is not +0 bit for bit — any of the five of a
 * padded column (quad padding, plain padding), ybar of a quad's tangent channels, the fourth gbar float of any column.  Every pointer
 * except cfg and weights is a device pointer.  mode, n_global, weights, alpha, cot (4 floats) as in dudf_loss_backward; the
 * `deterministic` option applies.  workspace: dudf_workspace_bytes_hess(cfg, n, n_hess).  Arrived after ABI 8 without changing any
 * existing signature.
 *   Refusals, all before any device work and in this order: weights NULL: DUDF_E_BADCFG; a mode that is none of the three, loss_s2
 *   without out_stats, n_hess != 0 outside loss_s1 with a Hessian weight: DUDF_E_BADMODE; a bad cfg, n < 0, n_hess > n: DUDF_E_BADCFG;
 *   workspace: DUDF_E_WORKSPACE; n_global < 1 with n > 0: DUDF_E_BADCFG; n == 0: nothing is launched, 0; any other NULL pointer the
 *   mode needs (h and out_hbar only with n_hess > 0, stats_in never): DUDF_E_BADCFG. */
int dudf_debug_loss_stage(const dudf_net_cfg* cfg, int mode, int64_t n, int64_t n_hess, const float* y, const float* g, const float* h,
                          const float* normals, const float* sdf, int64_t n_global, const double* weights, double alpha,
                          const float* cot, const double* stats_in, float* out_terms, double* out_stats, float* out_ybar,
                          float* out_gbar, float* out_hbar, int* out_pad_nonzero, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Host-only diagnostic (no GPU work): where the per-column arrays of a training workspace sit.  out (host, 10 values):
 * byte offsets of S, C, Q, E, A, Z, R, ZS in the workspace (order of `which` above), then the byte stride between two
 * feature-quad rows and between two layers OF THE fp32 ARRAYS.  Every offset and both strides are multiples of 256: a lane
 * quarter's 256-byte segment is exactly two cache lines (tests/test_cabi_symbols.py holds the layout to that). */
int dudf_debug_stash_layout(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess, int64_t* out);

/* Host-only diagnostic (nothing is launched): the kernel a launch of this workspace gets under the CURRENT options.
 * which: 0..3 the forward / reverse / adjoint forward / adjoint reverse sweep of the plain columns, 4..7 of the Hessian quads,
 *        8 the third-order jets; | DUDF_CHOICE_PAIR (0..3 only): the one-grid launch of quads + plain columns — DUDF_E_UNSUPPORTED
 *        means the two ranges are launched one after the other; DUDF_CHOICE_WGRAD: the hidden layers' weight-gradient GEMM.
 * flags: 1 = the forward sweep keeps h, 2 = keeps cos, 4 = training stores, 8 = the adjoint forward sweep ran (df/dx terms),
 *        16 = a query workspace (dudf_workspace_bytes_query) instead of a training one.
 * name: the kernel's name as a profiler prints it, without namespace and argument list, e.g. sweep_f16p_np_kernel<256,0,3>.
 * Returns 0, or the error the launch would return (DUDF_E_UNSUPPORTED / DUDF_E_BADMODE; `name` is then empty). */
#define DUDF_CHOICE_PAIR 16
#define DUDF_CHOICE_WGRAD (-1)
int dudf_debug_kernel_choice(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess, int which, int flags, char* name, size_t name_len);

/* Format of the stash a training workspace of this network and batch keeps between the sweeps and the weight-gradient GEMM
 * (the activations `backward()` needs — what autograd saves for reference src/model.py:116-135 / src/diff_operators.py:208-212),
 * as a bit mask of the arrays held at 24 bits, 12 bytes per 4 values, tile-major [layer][feature/16][column/16][64 lanes][3 dwords]:
 *   bit 1 (2) = R, E — read only by the adjoint sweeps — as fp32 values rounded to their top three bytes (16 significant bits: relative error <= 2^-16);
 *   bit 2 (4) = C = cos(w0 z_l) as FIXED POINT on a 2^-22 grid (absolute error <= 2^-23: the size of the sin/cos polynomials' own);
 *   bit 0 (1) = S, Q, A, Z — the weight-gradient GEMM's operands — as the same fixed point relative to a per-layer, per-COLUMN power of
 *               two 2^E the sweeps fix from a bound of the column (absolute error <= 2^(E-23); side arrays of 4 bytes per layer and
 *               column hold 2^E).  (ABI 5 stored these four as 24-bit FLOATS, 2^-17 of every value: that moved the 12-step trajectory
 *               by 4e-4; the fixed point holds every trajectory bar: tests/test_traj50_gpu.py.)
 *   0 = every array fp32, [layer][feature/4][column][4]  (option stash = 0; widths below 256; batches of 2^22 columns and more);
 *   6 = R, E, C (15 instead of 17 array-layer units per step): the default of round 4, and what 512-wide networks get (their kernel
 *       relays S, Q, A, Z through the stash — the next layer reads its operand back from there — and that relay stays fp32: as
 *       fixed point it held every single-step tolerance but not the 12-step trajectory, tests/test_traj512_gpu.py);
 *   7 = all seven (12.75 units): the default of 256-wide networks.  Every parity tolerance, the 12-step beetle trajectory and the
 *       50-step trajectory bars hold in it (tests/test_traj50_gpu.py, tests/test_stash_p24_gpu.py).
 * The answer is that of dudf_workspace_bytes_hess(cfg, n, n_hess)'s layout under the CURRENT options (the format depends on the
 * batch: 32-bit lane offsets inside a layer).  ZS is always fp32.  -1 = bad cfg.  dudf_debug_read_stash decodes every format. */
int dudf_stash_mode(const dudf_net_cfg* cfg, int64_t n, int64_t n_hess);

/* One training batch on the GPU — replaces `sampleTrainingData` (reference src/dataset.py:14-70, open3d on the CPU)
 * for a triangle soup tri (n_tri,9) and its precomputed surface cloud pc_pos/pc_nrm (n_pc,3) (reference
 * src/preprocess_mesh.py:39).  Writes THIS RANK's slice of the global batch [on | far | near] of
 * n_on + n_far + n_near points: x (n_l,3), normals (n_l,3) (zero off-surface), sdf (n_l) (zero on-surface,
 * unsigned distance otherwise); slice r of W of each stratum is [m*r/W, m*(r+1)/W).  Counter-based RNG keyed by
 * (seed, step): the union over ranks does not depend on W.
 * n_tri == 0 (tri may be NULL) selects the point-cloud-only variant, `sampleTrainingDataPC` (reference
 * src/dataset.py:80-131): far sdf = distance to the nearest cloud point (:72-78), near sdf = |offset| (:108-110). */
int dudf_sample_batch(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc,
                      int64_t n_on, int64_t n_far, int64_t n_near, uint64_t seed, uint64_t step, int rank, int world,
                      float* x, float* normals, float* sdf, void* stream);
/* The same batch with the step counter read from DEVICE memory when the kernel runs (*step_dev >= 0; not advanced by the call):
 * the graph-replayable form, bit-identical to dudf_sample_batch(step = *step_dev). */
int dudf_sample_batch_at(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc,
                         int64_t n_on, int64_t n_far, int64_t n_near, uint64_t seed, const int64_t* step_dev, int rank, int world,
                         float* x, float* normals, float* sdf, void* stream);

/* The same batches with the distances taken through an index instead of a scan of the whole shape, for meshes and clouds whose
 * size makes the scan the step's largest cost.  csrc/dudf_sample_indexed.hip, csrc/dudf_groupwalk.h; the cloud index: csrc/dudf_bvh.hip.  Like the dudf_mesh_* entry
 * points these arrived after ABI 8 without changing any existing signature.
 *
 * The cloud index is the mesh index's fixed-shape Morton tree over pc_pos (n_pc,3): a sorted copy of the points as 16-byte rows,
 * leaves of 8 points, fp32 boxes in heap order with empty boxes past the last leaf.  0 < n_pc < 2^31 (n_pc <= 0: DUDF_E_BADCFG,
 * larger: DUDF_E_UNSUPPORTED); the buffer is 256-byte aligned device memory of dudf_cloud_index_bytes(n_pc) bytes (else
 * DUDF_E_WORKSPACE).
 * dudf_cloud_index_bytes — size of the index of n_pc points; 0 for an n_pc out of range.
 * dudf_cloud_morton_codes — codes (n_pc) int64 = 63-bit Morton code of every point inside the bounding box of all of them.  The
 *   caller sorts them — a STABLE sort — and passes the permutation on.  Uses the head of `index` as scratch.
 * dudf_cloud_index_build — builds the index for `order` (n_pc) int64, order[s] = original index of the s-th point along the curve;
 *   any permutation gives a correct index.  Nothing comes back to the host; the 32-bit word at byte DUDF_MESH_INDEX_FLAGS_OFFSET
 *   of the index then holds DUDF_MESH_FLAG_NONFINITE if a coordinate is NaN or infinite and DUDF_MESH_FLAG_BAD_ORDER if an entry
 *   of `order` lies outside [0, n_pc); an index with a flag set must not be used.  Two builds from the same inputs are
 *   byte-identical.
 * dudf_sample_batch_indexed / dudf_sample_batch_indexed_at — dudf_sample_batch / dudf_sample_batch_at: the same arguments, samples,
 *   sharding and layout, and the same bits in x, normals and sdf (every distance is the minimum of the same exact fp64 values; a
 *   subtree is skipped only on a safe-side bound STRICTLY above the best exact value).  8 adjacent lanes share a sample and walk
 *   the tree together, a leaf per step.  n_tri > 0: far and near samples walk mesh_index, the index dudf_mesh_index_build wrote for
 *   tri (mesh_index_bytes = dudf_mesh_index_bytes(n_tri)); cloud_index is not looked at.  n_tri == 0: far samples walk cloud_index,
 *   built for pc_pos (cloud_index_bytes = dudf_cloud_index_bytes(n_pc)); near samples need no distance; mesh_index is not looked
 *   at.  On-surface samples walk nothing.  *out_stats (device int64, may be NULL, ADDED to) = exact evaluations of the call.
 *   Every check is made before the first device call: dudf_sample_batch's refusals; n_tri >= 2^31, or n_tri == 0 and
 *   n_pc >= 2^31: DUDF_E_UNSUPPORTED; then the index the mode needs — (NULL, 0 bytes), the caller has none: DUDF_E_BADCFG; NULL
 *   otherwise, misaligned, or not exactly the published size: DUDF_E_WORKSPACE.  The launch allocates nothing, copies nothing to
 *   the host and does not synchronise: both forms can be captured in a graph, the _at form drawing a new batch at every replay. */
size_t dudf_cloud_index_bytes(int64_t n_pc);
int dudf_cloud_morton_codes(const float* pc_pos, int64_t n_pc, void* index, size_t index_bytes, int64_t* codes, void* stream);
int dudf_cloud_index_build(const float* pc_pos, int64_t n_pc, const int64_t* order, void* index, size_t index_bytes, void* stream);
int dudf_sample_batch_indexed(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc, int64_t n_on,
                              int64_t n_far, int64_t n_near, uint64_t seed, uint64_t step, int rank, int world,
                              const void* mesh_index, size_t mesh_index_bytes, const void* cloud_index, size_t cloud_index_bytes,
                              float* x, float* normals, float* sdf, int64_t* out_stats, void* stream);
int dudf_sample_batch_indexed_at(const float* tri, int64_t n_tri, const float* pc_pos, const float* pc_nrm, int64_t n_pc, int64_t n_on,
                                 int64_t n_far, int64_t n_near, uint64_t seed, const int64_t* step_dev, int rank, int world,
                                 const void* mesh_index, size_t mesh_index_bytes, const void* cloud_index, size_t cloud_index_bytes,
                                 float* x, float* normals, float* sdf, int64_t* out_stats, void* stream);

/* Measurement hook (bench.py): while enabled, every kernel the library launches is bracketed by HIP
 * events ON THE STREAM IT IS LAUNCHED ON.  dudf_profile_dump synchronises those events and writes one
 * text line per kernel kind, "<name> <launches> <total_ms>\n", into buf (host), then clears the log. */
int dudf_profile_enable(int on);
int dudf_profile_dump(char* buf, size_t buflen);
/* "<kernel> <MHz>" per line: the shader clock the chip held under each MFMA kernel of the last profiled launches (ratio of
 * s_memtime to the 100 MHz s_memrealtime over the lifetime of the kernel's first workgroup).  Every roofline fraction
 * depends on it: the nominal peaks assume 2.4 GHz. */
int dudf_profile_clocks(char* buf, size_t buflen);
/* "<kernel> <products>" per line: products per algorithmic multiply of the kernel the library last launched under that name —
 * 1 = f32-input MFMA, 3 = fp16 hi/lo split ("fp16x3"), 6 = three-piece bf16 split ("bf16x6"); written by the launchers at the
 * point of dispatch, so a roofline label cannot drift from what ran (bench.py multiplies its algorithmic flops with it). */
int dudf_profile_products(char* buf, size_t buflen);

/* Run-time options of the library: process-wide integers, read at every call (rounds 1-4 read environment variables once, at the
 * first call).  An option that changes the stash format or the kernel family must not change between a forward call and the
 * backward call on the same workspace, and the workspace size has to be asked for again afterwards.  Names and values:
 *   "deterministic"         0 | 1   one owner per cross-workgroup sum of the training path: bit-reproducible, slow (default 0)
 *   "split"                 1 = fp16 hi/lo operand split, three products (default) | 0 = exact three-piece bf16 split, six products
 *   "split_quads"           1 (default) | 0: the Hessian quads / jets on bf16x6 while the plain columns stay on fp16x3
 *   "sweep_family"          1 = 16-bit matrix cores where built (default) | 0 = f32-input MFMA kernels everywhere (A/B reference)
 *   "stash"                 requested stash mask: 7 (default) | 6 | 0 — see dudf_stash_mode for what a workspace actually gets
 *   "wgrad_family"          0 = cooperative-split GEMM (default) | 1 = f32-input MFMA | 2 = bf16x6 with a per-wave split
 *   "wgrad_tr"              0 (default) | 1: fp32 rows staged row-major + transposed LDS fragment reads
 *   "pair_launch"           1 (default) | 0: quads and plain columns of a training sweep as two launches
 *   "wgrad_buffers"         4 (default) | 3: LDS image buffers of the weight-gradient GEMM that reads the 24-bit operands (4: one flag
 *                           poll per stage instead of two; same numbers)
 *   "wgrad_max_workgroups"  8 .. 256 (default 256 = one workgroup per CU, a single resident round).  A multi-GPU step that overlaps its
 *                           gradient all-reduces with the GEMM of the next layer group sets 240 before its launches: the GEMM's
 *                           workgroups fill the register file of the CUs they run on, and the RCCL kernel queued beside them needs
 *                           CUs of its own (diffudf_amd/engine.py).
 * Return: 0, DUDF_E_BADMODE for an unknown name, DUDF_E_BADCFG for a value out of range.  dudf_reset_options restores the defaults.
 * (These replace what `torch.backends.*` / environment switches would be around the reference's autograd path; the reference
 * itself has no such knobs.) */
int dudf_set_option(const char* name, int value);
int dudf_get_option(const char* name, int* value);
int dudf_reset_options(void);
/* = dudf_set_option("wgrad_max_workgroups", n); kept from ABI 5 */
int dudf_set_wgrad_max_workgroups(int n);

/* library / build identification, host string */
const char* dudf_version(void);
/* Which kernels split their fp32 matmul operands into two fp16 pieces (three products, "fp16x3") instead of three bf16
 * pieces (six products, "bf16x6"): bits 0-3 = the plain columns' forward / reverse / adjoint-forward / adjoint-reverse sweeps,
 * bit 4 = the weight-gradient GEMM of the 256-wide tiles, bit 5 = the Hessian quads / jets.  Set by the options "split" and
 * "split_quads"; both modes are held to the same fp32 parity tolerances. */
int dudf_split_mode(void);

/* 1 when the hidden-layer matmuls of this network's plain-column sweeps run on the bf16 matrix cores with the exact
 * 3-way split (bf16x6, fp32-equivalent), 0 when they run on the f32-input MFMA (bench.py prices its roofline with it). */
int dudf_sweeps_bf16x6(const dudf_net_cfg* cfg);

#ifdef __cplusplus
}
#endif
#endif /* DUDF_HIP_H */
