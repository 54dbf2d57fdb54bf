// CAP-UDF cell extraction on the GPU — replaces the Python triple loop of reference src/render_mc.py:201-256
// `extract_mesh_CAP(ndf, grad, resolution)` (133 M cells at 512^3, one `mcubes.marching_cubes` call per active cell).
// It consumes the (N,N,N) distance field and (N,N,N,3) direction field `dudf_grid_fields` leaves in HBM:
//
//   cell (i,j,k) is ACTIVE when min(ndf over its 8 corners) <= threshold (0.008, :205, :213);
//   corner sign = sign of dot(grad[corner 000], grad[corner]) (:224), res = +-ndf;  if any res < 0 (:230) the cell is
//   run through marching cubes at iso 0 on its 2x2x2 values (:231) and its vertices are shifted by (i,j,k) (:236-238),
//   cells being emitted in i, j, k loop order; finally v / (N-1) * 2 - 1 (:252).
//
// `mcubes` is PyMCubes 0.1.4: third-party, absent here — the per-cell marching cubes is this build's own (vertex at the
// linear-interpolation point of every sign-changing edge, table constructed by tools/gen_mc_table.py; conventions in
// oracle/capudf_oracle.py, which is the parity target; parity with PyMCubes itself is unpinned).
//
// Mapping: this is HBM-bound index/compaction work, no matrix cores.  One thread per cell, k fastest, 256 consecutive
// cells per workgroup, so the emission order of the reference (i, j, k loops) is the linear cell order:
//   pass 1  count : 8 coalesced row reads of ndf per cell (neighbouring cells and rows hit L1/L2: ~4 B/cell from HBM),
//                   the 8 direction vectors only for active cells (a thin shell around the surface); per-workgroup
//                   totals (cells, vertices, triangles)
//   pass 2  scan  : exclusive scan of the workgroup totals (dudf_scan_totals_kernel<3>: one workgroup; <= 524 k entries at 512^3)
//   pass 3  emit  : the same per-cell evaluation, an in-workgroup exclusive scan (dudf_wg_scan), float64
//                   vertices and int64 triangle indices written at their final offsets — deterministic, no atomics.
// The caller reads the three totals between pass 2 and pass 3 to size the outputs.
#include "dudf_context.h"
#include "dudf_capcell.h"            // eval_cell and the count / emit kernels, over the addressing policy below

namespace {

// the dense (N,N,N) / (N,N,N,3) arrays: work item = linear cell index, k fastest; corner (ii, jj, kk) at (i + ii, j + jj, k + kk)
struct DenseAddr {
    const float* ndf; const float* grad;
    int64_t n, m;                                        // grid points / cells per side (m = n - 1)
    int64_t ncells;
    __device__ __forceinline__ bool locate(int64_t cell, int& i, int& j, int& k) const {
        if (cell >= ncells) return false;
        const int64_t ij = cell / m;
        k = (int)(cell % m); j = (int)(ij % m); i = (int)(ij / m);
        return true;
    }
    __device__ __forceinline__ int64_t corner(int i, int j, int k, int c) const {
        return ((int64_t)i * n + j) * n + k + (int64_t)(c & 1) * n * n + (int64_t)((c >> 1) & 1) * n + ((c >> 2) & 1);
    }
    __device__ __forceinline__ float value(int64_t p) const { return ndf[p]; }
    __device__ __forceinline__ const float* vector(int64_t p) const { return grad + p * 3; }
};

struct CapArgs { DenseAddr ad; CapWork w; };

int64_t cap_blocks(int64_t grid_n) { const int64_t m = grid_n - 1; return (m * m * m + CB - 1) / CB; }

// the one statement of the workspace's layout: sizes with a null base, places on the caller's
size_t carve_cap(void* ws, int64_t grid_n, CapArgs* a) {
    DudfByteCarver cv = dudf_carve(ws);
    const int64_t nb = cap_blocks(grid_n);
    a->w.off = cv.take<int64_t>(nb * 3); a->w.blk = cv.take<uint32_t>(nb * 3);
    return cv.o;
}

int fill_args(const float* ndf, const float* grad, int64_t grid_n, double threshold, void* ws, size_t bytes, CapArgs* a) {
    if (grid_n < 2 || grid_n > 2048 || !ndf || !grad) return DUDF_E_BADCFG;
    if (int rc = dudf_check_buffer(ws, bytes, carve_cap(ws, grid_n, a))) return rc;
    const int64_t m = grid_n - 1;
    a->ad = DenseAddr{ndf, grad, grid_n, m, m * m * m};
    a->w.n = grid_n; a->w.threshold = threshold;
    a->w.verts = nullptr; a->w.tris = nullptr; a->w.cells = nullptr;
    return 0;
}

}  // namespace

extern "C" {

size_t dudf_capudf_workspace_bytes(int64_t grid_n) {
    if (grid_n < 2 || grid_n > 2048) return 0;
    CapArgs a;
    return carve_cap(nullptr, grid_n, &a);
}

int dudf_capudf_count(const float* ndf, const float* grad, int64_t grid_n, double threshold, int64_t* out_counts,
                      void* workspace, size_t workspace_bytes, void* stream) {
    CapArgs a;
    int rc = fill_args(ndf, grad, grid_n, threshold, workspace, workspace_bytes, &a);
    if (rc) return rc;
    if (!out_counts) return DUDF_E_BADCFG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    const int64_t nb = cap_blocks(grid_n);
    DUDF_TRY(dudf_launch(capudf_count_kernel<DenseAddr>, dim3((unsigned)nb), dim3(CB), st, a.ad, a.w));
    return dudf_launch(dudf_scan_totals_kernel<3>, dim3(1), dim3(1024), st, a.w.blk, a.w.off, nb, out_counts);
}

int dudf_capudf_emit(const float* ndf, const float* grad, int64_t grid_n, double threshold, double* out_vertices,
                     int64_t* out_triangles, int64_t* out_cells, void* workspace, size_t workspace_bytes, void* stream) {
    CapArgs a;
    int rc = fill_args(ndf, grad, grid_n, threshold, workspace, workspace_bytes, &a);
    if (rc) return rc;
    if (!out_vertices || !out_triangles) return DUDF_E_BADCFG;
    a.w.verts = out_vertices; a.w.tris = out_triangles; a.w.cells = out_cells;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DudfProfScope prof(PROF_OTHER, st);
    return dudf_launch(capudf_emit_kernel<DenseAddr>, dim3((unsigned)cap_blocks(grid_n)), dim3(CB), st, a.ad, a.w);
}

}  // extern "C"
