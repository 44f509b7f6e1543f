// lightglue_amd — relative pose of calibrated pairs: 5-point essential-matrix RANSAC with a fixed hypothesis budget, then (R, t) by cheirality
// (lg_relpose_estimate; the definition is in include/lightglue_amd.h).  Four launches per call:
//   rp_compact   one workgroup per pair: the verifier's compaction (tv_compact_pair) and the pair's two cameras, checked, into a 48-byte record, its 64-bit key 0;
//   rp_solve     pairs x (H / 64) workgroups of one wave, one LANE per hypothesis: the lane draws 5 correspondences, forms their bearings and solves in fp64
//                (null space, the 10 x 20 constraint system, the hidden-variable 3 x 3 polynomial matrix, the degree-10 polynomial, its real roots by
//                derivative bracketing); up to 10 candidates as pixel-space F, unit norm, output form, 9 floats each, into the workspace (zeros where none);
//   rp_score     pairs x (10 H / 256) workgroups, one LANE per candidate: the verifier's tile loop (tv_score_tiles) and inlier test, the best of the pair by
//                one 64-bit atomicMax on (count, ~hypothesis, ~root);
//   rp_finalise  one workgroup per pair: the winner re-read from the workspace, the optional fp64 refit on the essential manifold, mask, count, F, E, and the
//                pose among the four decompositions by the cheirality count over the inliers.
// The per-lane arrays of the solver (the 10 x 20 system alone is 1600 bytes) are indexed at run time and live in scratch memory: profiles/relative_pose.md
// has the compiler's figures.  Everything shared with the verifier and the absolute pose is lg_ransac_common.h's: the compaction, the sampler, bearings, horner<N> (the
// degree-10 root finder over it is this file's), det3 / ata3, the tile scoring loop, the winner's key (PoseKey, publish_winner), the Hartley normalisation (here over bearings), the F refit up to its
// null vector, the keep-if-not-worse recount and the mask; the camera rule is lg_common.h's.  The refusals (check_estimator_call) and the workspace layout (RpLayout)
// are lg_host_call.h's.  What is the estimator's own is here: the 5-point solver, the projection onto the essential manifold, the decomposition and the cheirality count.
#include "lg_host_call.h"
#include "lg_kernels.h"
#include "lg_ransac_common.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr int RP_SOLVE_THREADS = 64, RP_ROOTS = LG_RELPOSE_ROOTS;
constexpr double RP_EPS_NULL = 1e-9, RP_EPS_ELIM = 1e-12;

struct RpExt { unsigned long long key; int bad; int pad; float cam0[4]; float cam1[4]; };      // 48 bytes per pair
static_assert(sizeof(RpExt) == 48, "lg_relpose_workspace_bytes counts 48 bytes");

struct RpArgs {
    int pair0, refine, hyps;
    unsigned seed; float t2;
    TvSource src;
    const float* cameras0; const float* cameras1;
    TvHeader* head; RpExt* ext; f32x4* corr; int* rows; float* cand;     // workspace ([pairs][hyps][10][9] floats: the caller's `candidates` if given)
    float* rotations; float* translations; float* essentials; float* models;
    unsigned char* inliers0; int* num_inliers; long long* matches0_out; int* best; int* in_front; int* status;
};

// ------------------------------------------------------------------ compaction: one workgroup per pair
__global__ __launch_bounds__(TV_THREADS) void rp_compact_kernel(RpArgs a) {
    const int pair = a.pair0 + blockIdx.x;
    const long long at = (long long)pair * a.src.n0;
    __shared__ int wsum[4];
    __shared__ double red4[4];
    TvHeader h = tv_compact_pair(a.src, pair, a.corr + at, a.rows + at, wsum, red4);
    if (threadIdx.x == 0) {
        const PairImages src = pair_images(a.src.px, pair);
        RpExt x{};
        if (src.ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { x.cam0[e] = a.cameras0[(long long)src.i0 * 4 + e]; x.cam1[e] = a.cameras1[(long long)src.i1 * 4 + e]; }
            x.bad = camera_ok(x.cam0) && camera_ok(x.cam1) ? 0 : 1;
        }
        if (x.bad) h.count = 0;                          // an empty pair to every later launch
        a.head[pair] = h;
        a.ext[pair] = x;
    }
}

// ------------------------------------------------------------------ the 5-point solver, fp64, one lane
// monomials.  linear: x y z 1.  quadratic (RP_QI[i][j] of two linear ones): xx xy xz x yy yz y zz z 1.  cubic (RP_CI[quadratic][linear]), the first ten
// eliminated: x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
__device__ const unsigned char RP_QI[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
__device__ const unsigned char RP_CI[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7},
                                               {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};

// Gauss-Jordan elimination of the leading R x R block of the R x C matrix m (row-major), row pivoting (the first largest entry); false if a pivot is not above eps
template <int R, int C> __device__ bool rp_eliminate(double* m, double eps) {
    for (int k = 0; k < R; ++k) {
        int piv = k;
        for (int i = k + 1; i < R; ++i) if (fabs(m[i * C + k]) > fabs(m[piv * C + k])) piv = i;
        if (piv != k) for (int c = k; c < C; ++c) { const double t = m[k * C + c]; m[k * C + c] = m[piv * C + c]; m[piv * C + c] = t; }
        const double p = m[k * C + k];
        if (!(fabs(p) > eps)) return false;
        for (int c = k; c < C; ++c) m[k * C + c] = m[k * C + c] / p;
        for (int i = 0; i < R; ++i) {
            if (i == k) continue;
            const double f = m[i * C + k];
            for (int c = k; c < C; ++c) m[i * C + c] = m[i * C + c] - f * m[k * C + c];
        }
    }
    return true;
}
// q = ea eb - ec ed of four entries of E = x N[0] + y N[1] + z N[2] + N[3] (quadratic, 10 coefficients)
__device__ void rp_minor(const double (&N)[4][9], int ea, int eb, int ec, int ed, double (&q)[10]) {
    for (int e = 0; e < 10; ++e) q[e] = 0.0;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) q[RP_QI[i][j]] += N[i][ea] * N[j][eb] - N[i][ec] * N[j][ed];
}
// the real roots of p (degree 10, p[10] != 0) in ascending order: the roots of the k-th derivative lie one in each interval between those of the (k + 1)-th.  Rolled over
// the derivative order, prev[] / root[] indexed at run time (the solver's arrays live in scratch anyway); lg_abspose.hip's ap_real_roots<N> is the same method fully
// unrolled, which P3P needs to stay out of scratch and which costs this kernel time at degree 10 (profiles/ab_ransac_steps.md): two root finders over one horner<N>
__device__ int rp_real_roots(const double (&p)[11], double (&root)[10]) {
    if (!(fabs(p[10]) > 0.0)) return 0;
    double bound = 0.0;
    for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(p[i] / p[10]));
    bound = bound + 1.0;                                 // Cauchy; the roots of every derivative lie inside it too (Gauss-Lucas)
    if (!isfinite(bound)) return 0;
    double prev[10];
    int nprev = 0, n = 0;
    for (int k = 9; k >= 0; --k) {
        // the k-th derivative, degree 10 - k, padded with zeros to degree 10: c and dc are indexed statically and stay in registers through the bisection
        // (the padding changes no bit: 0 z + c is c)
        double c[11], dc[11];
#pragma unroll
        for (int i = 0; i < 11; ++i) {
            double f = 0.0;
            if (i + k <= 10) {
                f = p[i + k];
                for (int j = 1; j <= k; ++j) f = f * (double)(i + j);
            }
            c[i] = f;
        }
#pragma unroll
        for (int i = 0; i < 10; ++i) dc[i] = c[i + 1] * (double)(i + 1);
        dc[10] = 0.0;
        n = 0;
        double lo = -bound, flo = horner<10>(c, lo);
        for (int s = 0; s <= nprev; ++s) {
            const double hi = s < nprev ? prev[s] : bound, fhi = horner<10>(c, hi);
            if ((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0)) {
                double a = lo, b = hi;
                for (int it = 0; it < 64; ++it) {
                    const double m = 0.5 * (a + b), fm = horner<10>(c, m);
                    if ((fm < 0.0) == (flo < 0.0)) a = m; else b = m;
                }
                double z = 0.5 * (a + b);
                for (int it = 0; it < 3; ++it) {
                    const double zn = z - horner<10>(c, z) / horner<10>(dc, z);
                    if (zn >= a && zn <= b) z = zn;
                }
                root[n++] = z;
            }
            lo = hi; flo = fhi;
        }
        for (int i = 0; i < n; ++i) prev[i] = root[i];
        nprev = n;
    }
    return n;
}
// the solutions (x, y, z) of five bearing correspondences q[i] = (x0, y0, x1, y1), ascending in z, and the basis N of E = x N[0] + y N[1] + z N[2] + N[3]
__device__ int rp_five_point(const double (&q)[5][4], double (&N)[4][9], double (&sol)[10][3]) {
    double a[5 * 9];
    for (int i = 0; i < 5; ++i) {
        const double x = q[i][0], y = q[i][1], u = q[i][2], v = q[i][3];
        double* r = a + 9 * i;
        r[0] = u * x; r[1] = u * y; r[2] = u; r[3] = v * x; r[4] = v * y; r[5] = v; r[6] = x; r[7] = y; r[8] = 1.0;
    }
    if (!rp_eliminate<5, 9>(a, RP_EPS_NULL)) return 0;
    for (int k = 0; k < 4; ++k) {
        for (int e = 0; e < 9; ++e) N[k][e] = e < 5 ? -a[e * 9 + 5 + k] : (e == 5 + k ? 1.0 : 0.0);
        for (int j = 0; j < k; ++j) {                    // modified Gram-Schmidt
            double d = 0.0;
            for (int e = 0; e < 9; ++e) d += N[k][e] * N[j][e];
            for (int e = 0; e < 9; ++e) N[k][e] = N[k][e] - d * N[j][e];
        }
        double s = 0.0;
        for (int e = 0; e < 9; ++e) s += N[k][e] * N[k][e];
        s = sqrt(s);
        for (int e = 0; e < 9; ++e) N[k][e] = N[k][e] / s;
    }
    // G = E E^T (6 quadratics: 00 01 02 11 12 22), then G - tr(G) / 2 on the diagonal
    double G[6][10];
    const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double* g = G[sym[i][j]];
            for (int e = 0; e < 10; ++e) g[e] = 0.0;
            for (int k = 0; k < 3; ++k)
                for (int l1 = 0; l1 < 4; ++l1) for (int l2 = 0; l2 < 4; ++l2) g[RP_QI[l1][l2]] += N[l1][3 * i + k] * N[l2][3 * j + k];
        }
    for (int e = 0; e < 10; ++e) {
        const double half = 0.5 * ((G[0][e] + G[3][e]) + G[5][e]);
        G[0][e] -= half; G[3][e] -= half; G[5][e] -= half;
    }
    double M[10 * 20];
    for (int e = 0; e < 200; ++e) M[e] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double* row = M + 20 * (3 * i + j);
            for (int k = 0; k < 3; ++k) {
                const double* g = G[sym[i][k]];
                for (int e = 0; e < 10; ++e) for (int l = 0; l < 4; ++l) row[RP_CI[e][l]] += g[e] * N[l][3 * k + j];
            }
        }
    {   // det E = e0 (e4 e8 - e5 e7) - e1 (e3 e8 - e5 e6) + e2 (e3 e7 - e4 e6)
        double* row = M + 20 * 9;
        double mq[10];
        rp_minor(N, 4, 8, 5, 7, mq);
        for (int e = 0; e < 10; ++e) for (int l = 0; l < 4; ++l) row[RP_CI[e][l]] += mq[e] * N[l][0];
        rp_minor(N, 3, 8, 5, 6, mq);
        for (int e = 0; e < 10; ++e) for (int l = 0; l < 4; ++l) row[RP_CI[e][l]] -= mq[e] * N[l][1];
        rp_minor(N, 3, 7, 4, 6, mq);
        for (int e = 0; e < 10; ++e) for (int l = 0; l < 4; ++l) row[RP_CI[e][l]] += mq[e] * N[l][2];
    }
    if (!rp_eliminate<10, 20>(M, RP_EPS_ELIM)) return 0;
    // z (row of x2, y2, xy) - (row of x2z, y2z, xyz): three rows of B(z) (x, y, 1)^T = 0, coefficients ascending in z
    double bx[3][4], by[3][4], b1[3][5];
    for (int r = 0; r < 3; ++r) {
        const double* hi = M + 20 * (5 + 2 * r) + 10;
        const double* lo = M + 20 * (4 + 2 * r) + 10;
        bx[r][0] = -lo[2]; bx[r][1] = hi[2] - lo[1]; bx[r][2] = hi[1] - lo[0]; bx[r][3] = hi[0];
        by[r][0] = -lo[5]; by[r][1] = hi[5] - lo[4]; by[r][2] = hi[4] - lo[3]; by[r][3] = hi[3];
        b1[r][0] = -lo[9]; b1[r][1] = hi[9] - lo[8]; b1[r][2] = hi[8] - lo[7]; b1[r][3] = hi[7] - lo[6]; b1[r][4] = hi[6];
    }
    double p[11];
    for (int e = 0; e < 11; ++e) p[e] = 0.0;
    for (int r = 0; r < 3; ++r) {
        const int s = (r + 1) % 3, t = (r + 2) % 3;
        double m6[7];
        for (int e = 0; e < 7; ++e) m6[e] = 0.0;
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m6[i + j] += bx[s][i] * by[t][j] - bx[t][i] * by[s][j];
        for (int i = 0; i < 7; ++i) for (int j = 0; j < 5; ++j) p[i + j] += m6[i] * b1[r][j];
    }
    double root[10];
    const int n = rp_real_roots(p, root);
    for (int k = 0; k < n; ++k) {
        const double z = root[k];
        double v[3][3];
        for (int r = 0; r < 3; ++r) { v[r][0] = horner<3>(bx[r], z); v[r][1] = horner<3>(by[r], z); v[r][2] = horner<4>(b1[r], z); }
        double best[3] = {0.0, 0.0, 0.0}, len = -1.0;
        for (int r = 0; r < 3; ++r) {                    // the row pairs (0, 1), (0, 2), (1, 2)
            const int i = r == 2 ? 1 : 0, j = r == 0 ? 1 : 2;
            const double c0 = v[i][1] * v[j][2] - v[i][2] * v[j][1], c1 = v[i][2] * v[j][0] - v[i][0] * v[j][2], c2 = v[i][0] * v[j][1] - v[i][1] * v[j][0];
            const double l = (c0 * c0 + c1 * c1) + c2 * c2;
            if (l > len) { len = l; best[0] = c0; best[1] = c1; best[2] = c2; }
        }
        sol[k][0] = best[0] / best[2]; sol[k][1] = best[1] / best[2]; sol[k][2] = z;
    }
    return n;
}

// the candidate of an essential matrix: F = K1^-T E K0^-1 in fp64, rounded to float32, unit norm, output form; false (and all zero) if it is not finite
__device__ bool rp_candidate(const double (&E)[9], const float* cam0, const float* cam1, float (&m)[9]) {
    const double fx0 = cam0[0], fy0 = cam0[1], cx0 = cam0[2], cy0 = cam0[3], fx1 = cam1[0], fy1 = cam1[1], cx1 = cam1[2], cy1 = cam1[3];
    double g[9];
    for (int r = 0; r < 3; ++r) {
        const double a = E[3 * r] / fx0, b = E[3 * r + 1] / fy0;
        g[3 * r] = a; g[3 * r + 1] = b; g[3 * r + 2] = (E[3 * r + 2] - cx0 * a) - cy0 * b;
    }
    for (int c = 0; c < 3; ++c) {
        const double a = g[c] / fx1, b = g[3 + c] / fy1;
        m[c] = (float)a; m[3 + c] = (float)b; m[6 + c] = (float)((g[6 + c] - cx1 * a) - cy1 * b);
    }
    return tv_unit(m);
}

__global__ __launch_bounds__(RP_SOLVE_THREADS) void rp_solve_kernel(RpArgs a) {
    const int pair = a.pair0 + blockIdx.x, hyp = blockIdx.y * RP_SOLVE_THREADS + threadIdx.x;
    const TvHeader h = a.head[pair];
    float* out = a.cand + ((long long)pair * a.hyps + hyp) * (RP_ROOTS * 9);
    int n = 0;
    double N[4][9], sol[10][3];
    const RpExt x = a.ext[pair];
    if (h.count >= 5) {
        const f32x4* corr = a.corr + (long long)pair * a.src.n0;
        int pick[5];
        tv_sample<5>(a.seed, (unsigned)hyp, h.count, pick);
        double q[5][4];
        for (int i = 0; i < 5; ++i) {
            const f32x4 b = bearings(corr[pick[i]], x.cam0, x.cam1);
            for (int e = 0; e < 4; ++e) q[i][e] = b[e];
        }
        n = rp_five_point(q, N, sol);
    }
    for (int k = 0; k < RP_ROOTS; ++k) {
        float m[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (k < n) {
            double E[9];
            for (int e = 0; e < 9; ++e) E[e] = ((sol[k][0] * N[0][e] + sol[k][1] * N[1][e]) + sol[k][2] * N[2][e]) + N[3][e];
            rp_candidate(E, x.cam0, x.cam1, m);
        }
        for (int e = 0; e < 9; ++e) out[k * 9 + e] = m[e];
    }
}

// ------------------------------------------------------------------ scoring: one lane per candidate
__global__ __launch_bounds__(TV_THREADS) void rp_score_kernel(RpArgs a) {
    __shared__ f32x4 tile[TV_TILE];
    const int pair = a.pair0 + blockIdx.x, tid = threadIdx.x, c = blockIdx.y * TV_THREADS + tid, hyp = c / RP_ROOTS, root = c % RP_ROOTS;
    const int S = a.head[pair].count;
    if (S < 5) return;                                   // uniform per workgroup: the key stays 0
    const f32x4* corr = a.corr + (long long)pair * a.src.n0;
    const float* src = a.cand + ((long long)pair * a.hyps * RP_ROOTS + c) * 9;
    float m[1][9];
    bool any = false;
#pragma unroll
    for (int e = 0; e < 9; ++e) { m[0][e] = src[e]; any = any || src[e] != 0.f; }
    const bool valid = any && tv_finite9(m[0]);
    int pos[1] = {0}, neg[1] = {0};
    tv_score_tiles<TV_F, 1>(m, corr, S, a.t2, tile, pos, neg);
    const int count = valid ? pos[0] : 0;
    publish_winner(PoseKey::make(count, hyp, root), &a.ext[pair].key);
}

// ------------------------------------------------------------------ finalise: one workgroup per pair
// E <- E (v1 v1^T + v2 v2^T) with both singular values 1 (v1, v2 the two largest eigenvectors of E^T E).  One lane; J3, V3: 9 doubles each
__device__ bool rp_project_essential(double (&E)[9], double* J3, double* V3) {
    ata3(E, J3);
    const int c3 = tv_jacobi(J3, V3, 3);
    double out[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = true;
    for (int col = 0; col < 3; ++col) {
        if (col == c3) continue;
        const double v[3] = {V3[col], V3[3 + col], V3[6 + col]};
        double w[3];
        for (int r = 0; r < 3; ++r) w[r] = (E[3 * r] * v[0] + E[3 * r + 1] * v[1]) + E[3 * r + 2] * v[2];
        const double s = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
        ok = ok && s > 0.0 && isfinite(s);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) out[3 * r + c] += (w[r] / s) * v[c];
    }
    for (int e = 0; e < 9; ++e) E[e] = out[e];
    return ok;
}
// R <- R (3 I - R^T R) / 2
__device__ void rp_orthonormalise(double (&R)[9]) {
    double A[9], out[9];
    for (int p = 0; p < 3; ++p) for (int q = 0; q < 3; ++q) A[p * 3 + q] = (p == q ? 3.0 : 0.0) - ((R[p] * R[q] + R[3 + p] * R[3 + q]) + R[6 + p] * R[6 + q]);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) out[3 * r + c] = 0.5 * ((R[3 * r] * A[c] + R[3 * r + 1] * A[3 + c]) + R[3 * r + 2] * A[6 + c]);
    for (int e = 0; e < 9; ++e) R[e] = out[e];
}
// the two rotations and t0 of E (any scale).  One lane
__device__ void rp_decompose(const float (&e32)[9], double (&Ra)[9], double (&Rb)[9], double (&t0)[3], double* J3, double* V3) {
    double e[9], sq = 0.0;
    for (int i = 0; i < 9; ++i) { e[i] = (double)e32[i]; sq += e[i] * e[i]; }
    const double sc = 1.4142135623730951 / sqrt(sq);
    for (int i = 0; i < 9; ++i) e[i] = e[i] * sc;
    for (int p = 0; p < 3; ++p) for (int q = 0; q < 3; ++q) J3[p * 3 + q] = (e[3 * p] * e[3 * q] + e[3 * p + 1] * e[3 * q + 1]) + e[3 * p + 2] * e[3 * q + 2];
    const int c3 = tv_jacobi(J3, V3, 3);
    t0[0] = V3[c3]; t0[1] = V3[3 + c3]; t0[2] = V3[6 + c3];
    double big = t0[0];
    for (int i = 1; i < 3; ++i) big = fabs(t0[i]) > fabs(big) ? t0[i] : big;
    const double nrm = sqrt((t0[0] * t0[0] + t0[1] * t0[1]) + t0[2] * t0[2]) * (big < 0.0 ? -1.0 : 1.0);
    for (int i = 0; i < 3; ++i) t0[i] = t0[i] / nrm;
    ata3(e, J3);
    const int d3 = tv_jacobi(J3, V3, 3);
    const double v3[3] = {V3[d3], V3[3 + d3], V3[6 + d3]};
    // with E = U diag(s1, s2, s3) V^T: -+[t0]x E + s t0 v3^T = U (W^T or W) diag(s1, s2, 1) V^T for the sign s that makes the determinant positive
    for (int c = 0; c < 3; ++c) {
        const double te0 = t0[1] * e[6 + c] - t0[2] * e[3 + c], te1 = t0[2] * e[c] - t0[0] * e[6 + c], te2 = t0[0] * e[3 + c] - t0[1] * e[c];
        Ra[c] = t0[0] * v3[c] - te0; Ra[3 + c] = t0[1] * v3[c] - te1; Ra[6 + c] = t0[2] * v3[c] - te2;
        Rb[c] = t0[0] * v3[c] + te0; Rb[3 + c] = t0[1] * v3[c] + te1; Rb[6 + c] = t0[2] * v3[c] + te2;
    }
    const double da = det3<double>(Ra, Ra + 3, Ra + 6), db = det3<double>(Rb, Rb + 3, Rb + 6);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            if (da < 0.0) Ra[3 * r + c] = Ra[3 * r + c] - 2.0 * (t0[r] * v3[c]);
            if (db < 0.0) Rb[3 * r + c] = Rb[3 * r + c] - 2.0 * (t0[r] * v3[c]);
        }
    rp_orthonormalise(Ra);
    rp_orthonormalise(Rb);
}

__global__ __launch_bounds__(TV_THREADS) void rp_finalise_kernel(RpArgs a) {
    __shared__ unsigned char mask[LG_MAX_KEYPOINTS];
    __shared__ float model[9], ess[9];
    __shared__ int red8[8], red16[16], flag;
    __shared__ double red4[4], JA[81], JV[81], J3[9], V3[9], pose[2 * 9 + 3];
    const int pair = a.pair0 + blockIdx.x, tid = threadIdx.x, n0 = a.src.n0;
    const bool ok = pair_images(a.src.px, pair).ok;
    const TvHeader h = a.head[pair];
    const RpExt x = a.ext[pair];
    const int S = h.count;
    const long long at = (long long)pair * n0;
    const f32x4* corr = a.corr + at; const int* rows = a.rows + at;
    const unsigned long long key = x.key;
    const int hyp = PoseKey::hyp_of(key), root = PoseKey::root_of(key);
    for (int i = tid; i < n0; i += TV_THREADS) mask[i] = 0;
    const auto to_bearings = [&x](const f32x4& c) { return bearings(c, x.cam0, x.cam1); };
    float fin[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) fin[e] = 0.f;
    TvCount cur{0, 1};
    if (key) {                                           // uniform per workgroup
        const float* src = a.cand + (((long long)pair * a.hyps + hyp) * RP_ROOTS + root) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) fin[e] = src[e];
        cur = tv_count<TV_F>(fin, corr, S, a.t2, red8);
        if (a.refine && cur.count >= 8) {
            const Hartley hn = hartley(corr, S, to_bearings, red4);          // of the bearings of either side over the whole list
            double f[9];
            tv_null_vector<TV_F>(fin, cur.sign, corr, S, a.t2, hn, to_bearings, JA, JV, red4, f);
            if (tid == 0) {
                tv_denormalise<TV_F, double>(f, hn);
                bool good = rp_project_essential(f, J3, V3);
                float ref[9];
                good = rp_candidate(f, x.cam0, x.cam1, ref) && good;
                for (int e = 0; e < 9; ++e) model[e] = ref[e];
                flag = good ? 1 : 0;
            }
            __syncthreads();
            if (flag) tv_keep_if_not_worse<TV_F>(model, corr, S, a.t2, red8, cur, fin);        // uniform
        }
    }
    const bool empty = !key || cur.count == 0;
    __syncthreads();                                     // mask[] is zeroed
    tv_mark_inliers<TV_F>(empty, fin, cur.sign, corr, rows, S, a.t2, mask);
    // E = K1^T F K0 of the returned F, unit norm, float32, output form; the two rotations and t0 of it
    if (tid == 0) {
        float e32[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool good = false;
        if (!empty) {
            const double fx0 = x.cam0[0], fy0 = x.cam0[1], cx0 = x.cam0[2], cy0 = x.cam0[3], fx1 = x.cam1[0], fy1 = x.cam1[1], cx1 = x.cam1[2], cy1 = x.cam1[3];
            double g[9], E[9], sq = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double f0 = fin[3 * r], f1 = fin[3 * r + 1], f2 = fin[3 * r + 2];
                g[3 * r] = f0 * fx0; g[3 * r + 1] = f1 * fy0; g[3 * r + 2] = (f0 * cx0 + f1 * cy0) + f2;
            }
            for (int c = 0; c < 3; ++c) { E[c] = fx1 * g[c]; E[3 + c] = fy1 * g[3 + c]; E[6 + c] = (cx1 * g[c] + cy1 * g[3 + c]) + g[6 + c]; }
            for (int e = 0; e < 9; ++e) sq += E[e] * E[e];
            const double nrm = sqrt(sq);
            good = nrm > 0 && isfinite(nrm);
            for (int e = 0; e < 9; ++e) { e32[e] = good ? (float)(E[e] / nrm) : 0.f; good = good && isfinite(e32[e]); }
            if (!good) for (int e = 0; e < 9; ++e) e32[e] = 0.f;
            tv_output_form(e32);
        }
        for (int e = 0; e < 9; ++e) ess[e] = e32[e];
        if (good) {
            double Ra[9], Rb[9], t0[3];
            rp_decompose(e32, Ra, Rb, t0, J3, V3);
            for (int e = 0; e < 9; ++e) { pose[e] = Ra[e]; pose[9 + e] = Rb[e]; }
            for (int e = 0; e < 3; ++e) pose[18 + e] = t0[e];
        }
        flag = good ? 1 : 0;
    }
    __syncthreads();                                     // mask[], ess[], pose[], flag
    tv_write_rows(n0, mask, a.src.matches0 + at, a.inliers0 + at, a.matches0_out ? a.matches0_out + at : nullptr);
    const bool posed = flag != 0;                        // uniform
    int front[4] = {0, 0, 0, 0};
    if (posed) {
        for (int k = tid; k < S; k += TV_THREADS) {
            const f32x4 c = corr[k];
            if (tv_test<TV_F>(fin, c, a.t2) != cur.sign) continue;
            const f32x4 b = to_bearings(c);
            const double b0[3] = {(double)b[0], (double)b[1], 1.0}, b1[3] = {(double)b[2], (double)b[3], 1.0};
            const double bb = (b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const double* R = pose + (d < 2 ? 0 : 9);
                const double sg = (d & 1) ? -1.0 : 1.0;
                const double t[3] = {sg * pose[18], sg * pose[19], sg * pose[20]};
                double av[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) av[r] = (R[3 * r] * b0[0] + R[3 * r + 1] * b0[1]) + R[3 * r + 2] * b0[2];
                const double aa = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2], ab = (av[0] * b1[0] + av[1] * b1[1]) + av[2] * b1[2];
                const double at_ = (av[0] * t[0] + av[1] * t[1]) + av[2] * t[2], bt = (b1[0] * t[0] + b1[1] * t[1]) + b1[2] * t[2];
                front[d] += (ab * bt - bb * at_ > 0.0 && aa * bt - ab * at_ > 0.0) ? 1 : 0;
            }
        }
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) front[d] += __shfl_xor(front[d], o, 64);
        if ((tid & 63) == 0) for (int d = 0; d < 4; ++d) red16[4 * (tid >> 6) + d] = front[d];
    }
    __syncthreads();
    if (tid == 0) {
        int bestd = 0, bestc = 0;
        if (posed) {
            bestc = -1;
            for (int d = 0; d < 4; ++d) {
                const int cnt = ((red16[d] + red16[4 + d]) + red16[8 + d]) + red16[12 + d];
                if (cnt > bestc) { bestc = cnt; bestd = d; }
            }
        }
        const double* R = pose + (bestd < 2 ? 0 : 9);
        const double sg = (bestd & 1) ? -1.0 : 1.0;
        for (int e = 0; e < 9; ++e) {
            a.models[(long long)pair * 9 + e] = empty ? 0.f : fin[e];
            a.essentials[(long long)pair * 9 + e] = ess[e];
            a.rotations[(long long)pair * 9 + e] = posed ? (float)R[e] : 0.f;
        }
        for (int e = 0; e < 3; ++e) a.translations[(long long)pair * 3 + e] = posed ? (float)(sg * pose[18 + e]) : 0.f;
        a.num_inliers[pair] = empty ? 0 : cur.count;
        a.in_front[pair] = posed ? bestc : 0;
        if (a.best) a.best[pair] = empty ? -1 : hyp;
        a.status[pair] = !ok ? LG_ERR_INDEX : x.bad ? LG_ERR_CAMERA : LG_OK;
    }
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_relpose_workspace_bytes(int64_t pairs, int32_t n0, int32_t num_hypotheses, uint32_t flags) {
    RpLayout L;
    return rp_layout(pairs, n0, num_hypotheses, flags, L) ? -1 : L.total;
}

int lg_relpose_estimate(const lg_relpose_io* io, void* hip_stream) {
    RpLayout L;
    if (const int rc = check_estimator_call("lg_relpose_estimate", "lg_relpose_workspace_bytes", io, L)) return rc;
    const bool indexed = io->flags & LG_FLAG_INDEXED;
    const int P = io->pairs, n0 = io->n0, n1 = io->n1;
    if (P == 0) return LG_OK;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(io->workspace);
    RpArgs a{};
    a.src.n0 = n0; a.src.n1 = n1;
    if (indexed) a.src.px = PairIndex{io->index0, io->index1, io->images0, io->images1};
    a.refine = (io->flags & LG_RELPOSE_REFINE) ? 1 : 0;
    a.hyps = io->num_hypotheses; a.seed = io->seed; a.t2 = io->threshold * io->threshold;
    a.src.kpts0 = io->kpts0; a.src.kpts1 = io->kpts1; a.src.num0 = io->num0; a.src.num1 = io->num1;
    a.src.matches0 = reinterpret_cast<const long long*>(io->matches0);
    a.cameras0 = io->cameras0; a.cameras1 = io->cameras1;
    a.head = reinterpret_cast<TvHeader*>(ws + L.head); a.ext = reinterpret_cast<RpExt*>(ws + L.ext);
    a.corr = reinterpret_cast<f32x4*>(ws + L.corr); a.rows = reinterpret_cast<int*>(ws + L.rows);
    a.cand = io->candidates ? io->candidates : reinterpret_cast<float*>(ws + L.cand);
    a.rotations = io->rotations; a.translations = io->translations; a.essentials = io->essentials; a.models = io->models;
    a.inliers0 = io->inliers0; a.num_inliers = io->num_inliers; a.matches0_out = reinterpret_cast<long long*>(io->matches0_out);
    a.best = io->best_hypothesis; a.in_front = io->num_in_front; a.status = io->status;
    return for_pair_launches(P, [&](int p0, int count) -> int {
        a.pair0 = p0;
        hipLaunchKernelGGL(rp_compact_kernel, dim3(count), dim3(TV_THREADS), 0, s, a);
        hipLaunchKernelGGL(rp_solve_kernel, dim3(count, a.hyps / RP_SOLVE_THREADS), dim3(RP_SOLVE_THREADS), 0, s, a);
        hipLaunchKernelGGL(rp_score_kernel, dim3(count, a.hyps * RP_ROOTS / TV_THREADS), dim3(TV_THREADS), 0, s, a);
        hipLaunchKernelGGL(rp_finalise_kernel, dim3(count), dim3(TV_THREADS), 0, s, a);
        HIPCHK(hipGetLastError());
        return LG_OK;
    });
}

}  // extern "C"
