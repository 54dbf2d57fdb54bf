// Lewiner's 33-case triangulation of one cube, shared by the host library (dudf_meshudf.cpp: MeshUDF and the signed raster
// driver) and the device kernels (dudf_mcsdf.hip): table descriptors, the ambiguity tests and the (case, configuration) ->
// triangle-list switch of reference src/marching_cubes/_marching_cubes_lewiner_cy.pyx (`the_big_switch` :1848 /
// `check_the_big_switch` :2125, `test_face` :2404, `test_internal` :2436).  Written once so that both sides decide a cube from
// the same text; every unit that includes it is built with floating-point contraction off (the tests are in double, products
// and sums rounded separately, as the reference's C does).
#ifndef DUDF_LEWINER_H
#define DUDF_LEWINER_H
#include <cstdint>

#if defined(__HIPCC__)
#define DUDF_LW_HD __host__ __device__ inline
#define DUDF_LW_TABLE __attribute__((address_space(3)))    // the device keeps the tables in LDS: reads of them are DS reads
#else
#define DUDF_LW_HD inline
#define DUDF_LW_TABLE
#endif

namespace dudf_lewiner {

enum LutId {
    EDGESRELX, EDGESRELY, EDGESRELZ, CASESCLASSIC, CASES,
    TILING1, TILING2, TILING3_1, TILING3_2, TILING4_1, TILING4_2, TILING5, TILING6_1_1, TILING6_1_2, TILING6_2, TILING7_1,
    TILING7_2, TILING7_3, TILING7_4_1, TILING7_4_2, TILING8, TILING9, TILING10_1_1, TILING10_1_1_, TILING10_1_2,
    TILING10_2, TILING10_2_, TILING11, TILING12_1_1, TILING12_1_1_, TILING12_1_2, TILING12_2, TILING12_2_, TILING13_1,
    TILING13_1_, TILING13_2, TILING13_2_, TILING13_3, TILING13_3_, TILING13_4, TILING13_5_1, TILING13_5_2, TILING14,
    TEST3, TEST4, TEST6, TEST7, TEST10, TEST12, TEST13, SUBCONFIG13, N_LUTS
};

struct Lut {
    const DUDF_LW_TABLE int8_t* v;                   // (no default initialisers: the device keeps an array of these in LDS)
    int l1, l2;
    DUDF_LW_HD int at(int i) const { return v[i]; }
    DUDF_LW_HD int at(int i, int j) const { return v[i * l1 + j]; }
    DUDF_LW_HD int at(int i, int j, int k) const { return v[(i * l1 + j) * l2 + k]; }
};

constexpr double kEps = 2.220446049250313e-16;      // the reference's "FLT_EPSILON" is np.spacing(1.0), a double (:36)

struct Tiling { int lut, sub, nt; };                 // sub < 0: two-index table [config][3 nt]; else [config][sub][3 nt]

DUDF_LW_HD int edge_of(const Lut* L, const Tiling& t, int config, int k) {
    return t.sub < 0 ? L[t.lut].at(config, k) : L[t.lut].at(config, t.sub, k);
}

// ---- Lewiner's ambiguity tests on the eight corner values v[0..7] (cube numbering of the tables).  V: anything indexable that
// yields doubles — a `const double*` on the host, a strided view of LDS on the device.
template <class V> DUDF_LW_HD bool face_test(const V& v, int face) {                     // :2404-2433
    static constexpr int kF[7][4] = {{0, 0, 0, 0}, {0, 4, 5, 1}, {1, 5, 6, 2}, {2, 6, 7, 3}, {3, 7, 4, 0}, {0, 3, 2, 1}, {4, 7, 6, 5}};
    const int af = face < 0 ? -face : face;
    const double A = v[kF[af][0]], B = v[kF[af][1]], C = v[kF[af][2]], D = v[kF[af][3]];
    const double d = A * C - B * D;
    if (d > -kEps && d < kEps) return face >= 0;
    return face * A * d >= 0;
}

template <class V> DUDF_LW_HD bool interior_test(const V& v, const Lut* L, int c, int config, int sub, int s) {       // :2436-2570
    double t, At = 0.0, Bt = 0.0, Ct = 0.0, Dt = 0.0;
    if (c == 4 || c == 10) {
        const double a = (v[4] - v[0]) * (v[6] - v[2]) - (v[7] - v[3]) * (v[5] - v[1]);
        const double b = v[2] * (v[4] - v[0]) + v[0] * (v[6] - v[2]) - v[1] * (v[7] - v[3]) - v[3] * (v[5] - v[1]);
        t = -b / (2 * a + kEps);
        if (t < 0 || t > 1) return s > 0;
        At = v[0] + (v[4] - v[0]) * t; Bt = v[3] + (v[7] - v[3]) * t; Ct = v[2] + (v[6] - v[2]) * t; Dt = v[1] + (v[5] - v[1]) * t;
    } else {
        int e = -1;
        if (c == 6) e = L[TEST6].at(config, 2);
        else if (c == 7) e = L[TEST7].at(config, 4);
        else if (c == 12) e = L[TEST12].at(config, 3);
        else if (c == 13) e = L[TILING13_5_1].at(config, sub, 0);
        // per reference edge: the two ends (t = p / (p - q + eps)) and the three parallel edges (from, to) of B, C, D
        static constexpr int kE[12][8] = {{0, 1, 3, 2, 7, 6, 4, 5}, {1, 2, 0, 3, 4, 7, 5, 6}, {2, 3, 1, 0, 5, 4, 6, 7},
                                   {3, 0, 2, 1, 6, 5, 7, 4}, {4, 5, 7, 6, 3, 2, 0, 1}, {5, 6, 4, 7, 0, 3, 1, 2},
                                   {6, 7, 5, 4, 1, 0, 2, 3}, {7, 4, 6, 5, 2, 1, 3, 0}, {0, 4, 3, 7, 2, 6, 1, 5},
                                   {1, 5, 0, 4, 3, 7, 2, 6}, {2, 6, 1, 5, 0, 4, 3, 7}, {3, 7, 2, 6, 1, 5, 0, 4}};
        if (e >= 0 && e < 12) {
            const int* k = kE[e];
            t = v[k[0]] / (v[k[0]] - v[k[1]] + kEps);
            At = 0;
            Bt = v[k[2]] + (v[k[3]] - v[k[2]]) * t; Ct = v[k[4]] + (v[k[5]] - v[k[4]]) * t; Dt = v[k[6]] + (v[k[7]] - v[k[6]]) * t;
        }
    }
    const int test = (At >= 0 ? 1 : 0) + (Bt >= 0 ? 2 : 0) + (Ct >= 0 ? 4 : 0) + (Dt >= 0 ? 8 : 0);
    switch (test) {
        case 5: return (At * Ct - Bt * Dt < kEps) ? s > 0 : false;          // (falls off the end otherwise: 0)
        case 10: return (At * Ct - Bt * Dt >= kEps) ? s > 0 : false;
        case 7: case 11: case 13: case 14: case 15: return s < 0;
        default: return s > 0;
    }
}

// (case, configuration) -> which triangle list applies (`the_big_switch` / `check_the_big_switch`, :1848-2395)
template <class V> DUDF_LW_HD Tiling resolve(const V& v, const Lut* L, int c, int config) {
    auto ft = [&](int f) { return face_test(v, f); };
    switch (c) {
        case 1: return {TILING1, -1, 1};
        case 2: return {TILING2, -1, 2};
        case 3: return ft(L[TEST3].at(config)) ? Tiling{TILING3_2, -1, 4} : Tiling{TILING3_1, -1, 2};
        case 4: return interior_test(v, L, c, config, 0, L[TEST4].at(config)) ? Tiling{TILING4_1, -1, 2} : Tiling{TILING4_2, -1, 6};
        case 5: return {TILING5, -1, 3};
        case 6:
            if (ft(L[TEST6].at(config, 0))) return {TILING6_2, -1, 5};
            return interior_test(v, L, c, config, 0, L[TEST6].at(config, 1)) ? Tiling{TILING6_1_1, -1, 3} : Tiling{TILING6_1_2, -1, 9};
        case 7: {
            int sub = 0;
            if (ft(L[TEST7].at(config, 0))) sub += 1;
            if (ft(L[TEST7].at(config, 1))) sub += 2;
            if (ft(L[TEST7].at(config, 2))) sub += 4;
            switch (sub) {
                case 0: return {TILING7_1, -1, 3};
                case 1: return {TILING7_2, 0, 5};
                case 2: return {TILING7_2, 1, 5};
                case 3: return {TILING7_3, 0, 9};
                case 4: return {TILING7_2, 2, 5};
                case 5: return {TILING7_3, 1, 9};
                case 6: return {TILING7_3, 2, 9};
                default: return interior_test(v, L, c, config, sub, L[TEST7].at(config, 3)) ? Tiling{TILING7_4_2, -1, 9} : Tiling{TILING7_4_1, -1, 5};
            }
        }
        case 8: return {TILING8, -1, 2};
        case 9: return {TILING9, -1, 4};
        case 10: case 12: {
            const int T = c == 10 ? TEST10 : TEST12;
            const int t11 = c == 10 ? TILING10_1_1 : TILING12_1_1, t11_ = c == 10 ? TILING10_1_1_ : TILING12_1_1_;
            const int t12 = c == 10 ? TILING10_1_2 : TILING12_1_2, t2 = c == 10 ? TILING10_2 : TILING12_2, t2_ = c == 10 ? TILING10_2_ : TILING12_2_;
            if (ft(L[T].at(config, 0))) return ft(L[T].at(config, 1)) ? Tiling{t11_, -1, 4} : Tiling{t2, -1, 8};
            if (ft(L[T].at(config, 1))) return {t2_, -1, 8};
            return interior_test(v, L, c, config, 0, L[T].at(config, 2)) ? Tiling{t11, -1, 4} : Tiling{t12, -1, 8};
        }
        case 11: return {TILING11, -1, 4};
        case 13: {
            int sub = 0;
            for (int k = 0; k < 6; ++k) if (ft(L[TEST13].at(config, k))) sub += 1 << k;
            sub = L[SUBCONFIG13].at(sub);
            if (sub == 0) return {TILING13_1, -1, 4};
            if (sub <= 6) return {TILING13_2, sub - 1, 6};
            if (sub <= 18) return {TILING13_3, sub - 7, 10};
            if (sub <= 22) return {TILING13_4, sub - 19, 12};
            if (sub <= 26) return interior_test(v, L, c, config, sub - 23, L[TEST13].at(config, 6)) ? Tiling{TILING13_5_1, sub - 23, 6}
                                                                                                  : Tiling{TILING13_5_2, sub - 23, 10};
            if (sub <= 38) return {TILING13_3_, sub - 27, 10};
            if (sub <= 44) return {TILING13_2_, sub - 39, 6};
            if (sub == 45) return {TILING13_1_, -1, 4};
            return {TILING13_1, -1, 0};               // "impossible case 13": nothing is added
        }
        case 14: return {TILING14, -1, 4};
        default: return {TILING1, -1, 0};
    }
}

}  // namespace dudf_lewiner
#endif
