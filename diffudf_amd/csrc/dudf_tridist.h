// Exact point-to-triangle distance, shared by the batch sampler (dudf_sample.hip) and the mesh-distance queries
// (dudf_meshdist.hip).  One arithmetic, so a distance the sampler writes and one a query returns come from the same expression.
#ifndef DUDF_TRIDIST_H
#define DUDF_TRIDIST_H

// squared distance from p to triangle (a,b,c): closest point by Voronoi regions of the triangle.  In fp64, like the
// oracle (and like nothing in fp32 can be: |p - c|^2 of coordinates ~1 carries 1e-7 absolute, 1e-4 of a near-surface
// distance of 1e-3); 2 k triangles x 2 k queries per step is noise for the fp64 vector pipe.
// (cx, cy, cz) = closest point - a.
__device__ __forceinline__ double tri_closest(double px, double py, double pz, const float* t, double& cx, double& cy, double& cz) {
    const double ax = t[0], ay = t[1], az = t[2];
    const double abx = t[3] - ax, aby = t[4] - ay, abz = t[5] - az;
    const double acx = t[6] - ax, acy = t[7] - ay, acz = t[8] - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double d1 = abx * apx + aby * apy + abz * apz;
    const double d2 = acx * apx + acy * apy + acz * apz;
    if (d1 <= 0.0 && d2 <= 0.0) { cx = cy = cz = 0.0; }
    else {
        const double bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
        const double d3 = abx * bpx + aby * bpy + abz * bpz;
        const double d4 = acx * bpx + acy * bpy + acz * bpz;
        if (d3 >= 0.0 && d4 <= d3) { cx = abx; cy = aby; cz = abz; }
        else {
            const double vc = d1 * d4 - d3 * d2;
            if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
                const double v = d1 / (d1 - d3);
                cx = v * abx; cy = v * aby; cz = v * abz;
            } else {
                const double cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
                const double d5 = abx * cpx + aby * cpy + abz * cpz;
                const double d6 = acx * cpx + acy * cpy + acz * cpz;
                if (d6 >= 0.0 && d5 <= d6) { cx = acx; cy = acy; cz = acz; }
                else {
                    const double vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
                        const double w = d2 / (d2 - d6);
                        cx = w * acx; cy = w * acy; cz = w * acz;
                    } else {
                        const double va = d3 * d6 - d5 * d4;
                        if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
                            const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                            cx = abx + w * (acx - abx); cy = aby + w * (acy - aby); cz = abz + w * (acz - abz);
                        } else {
                            const double den = 1.0 / (va + vb + vc);
                            const double v = vb * den, w = vc * den;
                            cx = abx * v + acx * w; cy = aby * v + acy * w; cz = abz * v + acz * w;
                        }
                    }
                }
            }
        }
    }
    const double dx = apx - cx, dy = apy - cy, dz = apz - cz;
    return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ double tri_dist2(double px, double py, double pz, const float* t) {
    double cx, cy, cz;
    return tri_closest(px, py, pz, t, cx, cy, cz);
}

#endif  // DUDF_TRIDIST_H
