// lightglue_amd — THE 3 x 3 elimination of the triangulator, the bundle adjuster and the positioner (include/lightglue_amd.h, lg_triangulate: "Start"), and
// the inverse by columns the two points kernels take from it: device code, static indices only (no scratch).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)      // the definition has no fused multiply-add; the including files say the same for what follows

namespace lg {

constexpr double TRI_EPS = 1e-12;

// M x = b for a symmetric 3 x 3 M given by its upper triangle; false on a pivot that is not above TRI_EPS times M's largest diagonal entry.  Static indices only
__device__ __forceinline__ bool tri_solve3(const double (&s)[6], const double (&b)[3], double (&x)[3]) {
    double M[3][4] = {{s[0], s[1], s[2], b[0]}, {s[1], s[3], s[4], b[1]}, {s[2], s[4], s[5], b[2]}};
    const double bar = TRI_EPS * fmax(fmax(s[0], s[3]), s[5]);
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int r = c + 1; r < 3; ++r) {
            const bool swap = fabs(M[r][c]) > fabs(M[c][c]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const double lo = M[c][j], hi = M[r][j]; M[c][j] = swap ? hi : lo; M[r][j] = swap ? lo : hi; }
        }
        ok = ok && fabs(M[c][c]) > bar;
#pragma unroll
        for (int r = c + 1; r < 3; ++r) {
            const double f = M[r][c] / M[c][c];
#pragma unroll
            for (int j = c + 1; j < 4; ++j) M[r][j] = M[r][j] - f * M[c][j];
        }
    }
    x[2] = M[2][3] / M[2][2];
    x[1] = (M[1][3] - M[1][2] * x[2]) / M[1][1];
    x[0] = ((M[0][3] - M[0][1] * x[1]) - M[0][2] * x[2]) / M[0][0];
    return ok && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// Mi = M^-1 of the same M, column by column through tri_solve3; false if any column's elimination fails (every column is still written)
__device__ __forceinline__ bool tri_inverse3(const double (&s)[6], double (&Mi)[3][3]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
        double x[3];
        ok = tri_solve3(s, e, x) && ok;
        Mi[0][c] = x[0]; Mi[1][c] = x[1]; Mi[2][c] = x[2];
    }
    return ok;
}

}  // namespace lg
