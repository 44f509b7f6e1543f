// lightglue_amd — lg_bundle_adjust_focal's back substitution and trial state (per iteration 4 of lg_bundle.hip's list).  A file of its own: a second
// caller of cholesky_backsolve in lg_bundle.hip changes the registers the compiler gives ba_backsolve_kernel there, and lg_bundle_adjust's kernels are to keep
// the instruction streams they had (profiles/bundle_adjust_focal.md).
#include <cmath>

#include "lg_bundle_args.h"
#include "lg_cholesky.h"
#include "lg_kernels.h"

#pragma clang fp contract(off)

namespace lg {

// ONE workgroup: L^T s = z backwards with 7 entries per image, the trial poses (ba_backsolve_kernel's Rodrigues step, written out again here: shared as a
// template, that kernel would not keep its instruction stream either) and the trial cameras, f <- f exp(d) for fx and fy of a free camera (a trial focal
// length that is not finite or not > 0 fails the step); a held column's step is 0
__global__ __launch_bounds__(BA_THREADS) void ba_backsolve_focal_kernel(BaFocalArgs a) {
    constexpr int D = 7;
    __shared__ double sd[D * LG_BA_MAX_IMAGES];
    __shared__ CholeskySolveLds m;
    if (a.head->converged) return;
    const int t = threadIdx.x;
    cholesky_backsolve(a.S, a.dim, 1, sd, m);
    const int s = a.head->sel;
    int bad = 0;
    for (int k = t; k < a.images; k += BA_THREADS) {
        const double* P = ba_pose(a, s, k);
        double* out = a.pose + ((long long)(s ^ 1) * a.images + k) * 12;
        const bool cf = ba_cam_free(a, k);
        const double d = cf ? sd[D * k + 6] : 0.0, scale = exp(d);
        const double* c0 = ba_cam<true>(a, s, k);
        double* c1 = a.cam + ((long long)(s ^ 1) * a.images + k) * 4;
        a.delta[k * D + 6] = d;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double v = cf ? c0[q] * scale : c0[q];
            if (cf && !(isfinite(v) && v > 0.0)) bad = 1;
            c1[q] = v; c1[2 + q] = c0[2 + q];
        }
        if (!ba_free(a, k)) {
            for (int q = 0; q < 12; ++q) out[q] = P[q];
            for (int q = 0; q < 6; ++q) a.delta[k * D + q] = 0.0;
            continue;
        }
        double x[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) { x[q] = sd[D * k + q]; a.delta[k * D + q] = x[q]; }
        // Rodrigues(w) = I + sin(th) [k]x + (1 - cos(th)) [k]x^2, k = w / th
        const double th = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
        double Q[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        if (th > 0.0) {
            const double kx = x[0] / th, ky = x[1] / th, kz = x[2] / th, sn = sin(th), c1 = 1.0 - cos(th);
            const double Kx[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double kk = (Kx[3 * i] * Kx[j] + Kx[3 * i + 1] * Kx[3 + j]) + Kx[3 * i + 2] * Kx[6 + j];
                    Q[3 * i + j] = (Q[3 * i + j] + sn * Kx[3 * i + j]) + c1 * kk;
                }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = (Q[3 * i] * P[j] + Q[3 * i + 1] * P[4 + j]) + Q[3 * i + 2] * P[8 + j];
                if (j == 3) v = v + x[3 + i];
                if (!isfinite(v)) bad = 1;
                out[4 * i + j] = v;
            }
    }
    if (bad) atomicOr(&a.head->fail, 1);
}

void ba_launch_backsolve_focal(const BaFocalArgs& a, hipStream_t s) { hipLaunchKernelGGL(ba_backsolve_focal_kernel, dim3(1), dim3(BA_THREADS), 0, s, a); }

}  // namespace lg
