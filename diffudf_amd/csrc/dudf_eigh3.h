// Symmetric 3x3 eigen-decomposition on the device, shared by the loss kernels (dudf_loss.hip) and the field features
// (dudf_query.hip).  Device code: not for dudf_math.h, which dudf_hostmath.c compiles as C.
#pragma once

// Symmetric 3x3 eigen-decomposition of the LOWER triangle (as torch.linalg.eigh reads it, reference
// src/loss_functions.py:142), cyclic Jacobi in fp64, eigenvalues ascending.  V[i][j] = component i of v_j.
__device__ __forceinline__ void eigh3(const double (&Hm)[3][3], double (&lam)[3], double (&V)[3][3]) {
    double A[3][3] = {{Hm[0][0], Hm[1][0], Hm[2][0]}, {Hm[1][0], Hm[1][1], Hm[2][1]}, {Hm[2][0], Hm[2][1], Hm[2][2]}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 10; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-34 * dia || off == 0.0) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = (pq == 2) ? 1 : 0, q = (pq == 0) ? 1 : 2;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
            const int r = 3 - p - q;
            const double app = A[p][p], aqq = A[q][q], arp = A[r][p], arq = A[r][q];
            A[p][p] = app - t * apq; A[q][q] = aqq + t * apq; A[p][q] = A[q][p] = 0.0;
            A[r][p] = A[p][r] = c * arp - sn * arq;
            A[r][q] = A[q][r] = sn * arp + c * arq;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double vip = V[i][p], viq = V[i][q];
                V[i][p] = c * vip - sn * viq;
                V[i][q] = sn * vip + c * viq;
            }
        }
    }
    lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
    auto swp = [&](int i, int j) {
        if (lam[i] > lam[j]) {
            const double t = lam[i]; lam[i] = lam[j]; lam[j] = t;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double u = V[k][i]; V[k][i] = V[k][j]; V[k][j] = u; }
        }
    };
    swp(0, 1); swp(1, 2); swp(0, 1);
}
