// lightglue_amd — two-view geometric verification of match lists: RANSAC with a fixed hypothesis budget for a homography or a fundamental matrix per pair
// (lg_twoview_verify; the definition is in include/lightglue_amd.h).  Three launches per call:
//   tv_compact     one workgroup per pair: matches0[p, :] -> the dense list of correspondences (x0, y0, x1, y1) in ascending order of the image-0 keypoint
//                  (wave ballot + prefix: the order is fixed), its length S_p, the Hartley normalisation of either side, the pair's key reset to 0;
//   tv_hypothesis  pairs x (H / 256) workgroups, one LANE per hypothesis: the lane draws its sample, solves it (up to 3 models of 9 floats in registers),
//                  the pair's correspondences stream through LDS in tiles of TV_TILE (every lane reads the same address: a broadcast), the score is the integer
//                  inlier count, and the best of the pair is one atomicMax on (count, ~hypothesis, ~root);
//   tv_finalise    one workgroup per pair: the winner recomputed from its hypothesis number, the optional fp64 least-squares refit, mask, count, model.
// What a pair reads is lg_common.h's (PairIndex / pair_images, live_rows), and so are the compaction round (compact_slot) and the fixed-order block sum of the fp64
// reductions (block_sum); the refusals (check_estimator_call), the workspace layout (TvLayout) and the cut of the pair list into launches are lg_host_call.h's.
// The compaction with its Hartley normalisation, the sampling hash, the model helpers, the inlier test, the tile scoring loop, the winner's key (TvKey,
// publish_winner), the refit up to its null vector (tv_null_vector), the keep-if-not-worse recount, the count and the mask steps are lg_ransac_common.h's: lg_relpose.hip
// runs the same code.  What is the verifier's own is here: the two minimal solvers, the rank-2 step of the F refit and the order of the launches.
// The solvers are compiled without floating-point contraction and the scoring is written in explicit fmaf: a model and a decision are the same bits in
// tv_hypothesis and tv_finalise, whatever the compiler would fuse in either.
#include "lg_host_call.h"
#include "lg_kernels.h"
#include "lg_ransac_common.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr float TV_EPS_H = 1e-3f, TV_EPS_F = 1e-4f, TV_EPS_CUBIC = 1e-8f, TV_EPS_ROOT = 1e-2f;

struct TvArgs {
    int pair0, kind, refine, given, hyps;
    unsigned seed; float t2;
    TvSource src;                                        // the stores, the pair index and matches0 (lg_twoview_common.h)
    const float* models_in;
    TvHeader* head; f32x4* corr; int* rows;              // workspace: [pairs], [pairs][n0], [pairs][n0]
    float* models; unsigned char* inliers0; int* num_inliers; long long* matches0_out; int* best; int* status;
};

// ------------------------------------------------------------------ compaction: one workgroup per pair
__global__ __launch_bounds__(TV_THREADS) void tv_compact_kernel(TvArgs a) {
    const int pair = a.pair0 + blockIdx.x;
    const long long at = (long long)pair * a.src.n0;
    __shared__ int wsum[4];
    __shared__ double red4[4];
    const TvHeader h = tv_compact_pair(a.src, pair, a.corr + at, a.rows + at, wsum, red4);
    if (threadIdx.x == 0) a.head[pair] = h;
}

// the projective basis of four points (x, y, 1): c[i] = the cross products of the first three, lam[i] = c[i] . p3, det = c[0] . p0; false below TV_EPS_H
__device__ __forceinline__ bool tv_basis(const float (&x)[4], const float (&y)[4], float (&c)[3][3], float (&lam)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        c[i][0] = y[j] - y[k]; c[i][1] = x[k] - x[j]; c[i][2] = x[j] * y[k] - y[j] * x[k];
        lam[i] = (c[i][0] * x[3] + c[i][1] * y[3]) + c[i][2];
    }
    const float det = (c[0][0] * x[0] + c[0][1] * y[0]) + c[0][2];
    return fminf(fminf(fabsf(lam[0]), fabsf(lam[1])), fminf(fabsf(lam[2]), fabsf(det))) > TV_EPS_H;
}
// the homography of 4 normalised correspondences q[i] = (x0, y0, x1, y1); normalised model out (not yet of unit norm)
__device__ __forceinline__ bool tv_solve_h(const f32x4 (&q)[4], float (&h)[9]) {
    float xs[4], ys[4], xd[4], yd[4], cs[3][3], ls[3], cd[3][3], ld[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) { xs[i] = q[i][0]; ys[i] = q[i][1]; xd[i] = q[i][2]; yd[i] = q[i][3]; }
    const bool ok0 = tv_basis(xs, ys, cs, ls), ok1 = tv_basis(xd, yd, cd, ld), ok = ok0 && ok1;
#pragma unroll
    for (int e = 0; e < 9; ++e) h[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const float w = ld[i] * (ls[j] * ls[k]);         // column i of B = ld[i] (xd, yd, 1)_i, row i of A^-1 = cs[i] ls[j] ls[k]
        const float b[3] = {w * xd[i], w * yd[i], w};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int col = 0; col < 3; ++col) h[3 * r + col] = h[3 * r + col] + b[r] * cs[i][col];
    }
    return ok;
}

// the null space of 7 normalised correspondences as N1 + z N2 (N1[7] = 1, N2[8] = 1) and the real roots z of det = 0; returns their number, 0 for an invalid sample;
// well[k]: root k is well conditioned
__device__ __forceinline__ int tv_solve_f(const f32x4 (&q)[7], float (&n1)[9], float (&n2)[9], float (&z)[3], bool (&well)[3]) {
    float a[7][9];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const float x = q[i][0], y = q[i][1], u = q[i][2], v = q[i][3];
        a[i][0] = u * x; a[i][1] = u * y; a[i][2] = u; a[i][3] = v * x; a[i][4] = v * y; a[i][5] = v; a[i][6] = x; a[i][7] = y; a[i][8] = 1.f;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int i = k + 1; i < 7; ++i) {                // the largest |a[i][k]|, i >= k, ends in row k (the first one on a tie)
            const bool sw = fabsf(a[i][k]) > fabsf(a[k][k]);
#pragma unroll
            for (int c = k; c < 9; ++c) { const float t = a[k][c]; a[k][c] = sw ? a[i][c] : t; a[i][c] = sw ? t : a[i][c]; }
        }
        ok = ok && fabsf(a[k][k]) > TV_EPS_F;
        const float piv = a[k][k];
#pragma unroll
        for (int c = k; c < 9; ++c) a[k][c] = a[k][c] / piv;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            if (i == k) continue;
            const float f = a[i][k];
#pragma unroll
            for (int c = k; c < 9; ++c) a[i][c] = a[i][c] - f * a[k][c];
        }
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) { n1[i] = -a[i][7]; n2[i] = -a[i][8]; }
    n1[7] = 1.f; n1[8] = 0.f; n2[7] = 0.f; n2[8] = 1.f;
    // det(N1 + z N2) = c0 + c1 z + c2 z^2 + c3 z^3 by multilinearity in the rows
    const float c0 = det3(n1, n1 + 3, n1 + 6), c3 = det3(n2, n2 + 3, n2 + 6);
    const float c1 = (det3(n2, n1 + 3, n1 + 6) + det3(n1, n2 + 3, n1 + 6)) + det3(n1, n1 + 3, n2 + 6);
    const float c2 = (det3(n1, n2 + 3, n2 + 6) + det3(n2, n1 + 3, n2 + 6)) + det3(n2, n2 + 3, n1 + 6);
    ok = ok && fabsf(c3) > TV_EPS_CUBIC;
    const float A = c2 / c3, B = c1 / c3, C = c0 / c3;
    const float Q = (A * A - 3.f * B) / 9.f, R = ((2.f * A * A * A - 9.f * A * B) + 27.f * C) / 54.f;
    const float Q3 = Q * Q * Q, R2 = R * R;
    int n;
    if (R2 < Q3) {
        const float th = acosf(fminf(fmaxf(R / sqrtf(Q3), -1.f), 1.f)), sq = -2.f * sqrtf(Q);
#pragma unroll
        for (int k = 0; k < 3; ++k) z[k] = sq * cosf((th + 6.2831853071795865f * (float)k) / 3.f) - A / 3.f;
        n = 3;
    } else {
        const float e = -copysignf(cbrtf(fabsf(R) + sqrtf(R2 - Q3)), R);
        const float g = e != 0.f ? Q / e : 0.f;
        z[0] = (e + g) - A / 3.f; z[1] = z[2] = 0.f;
        n = 1;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int it = 0; it < 2; ++it) {                 // Newton on the monic cubic
            const float p = ((z[k] + A) * z[k] + B) * z[k] + C, dp = (3.f * z[k] + 2.f * A) * z[k] + B;
            if (fabsf(dp) > 1e-20f) z[k] = z[k] - p / dp;
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                        // a (nearly) double root is lost to rounding: |p'(z)| against the size of its terms
        const float dp = (3.f * z[k] + 2.f * A) * z[k] + B;
        well[k] = fabsf(dp) > TV_EPS_ROOT * ((fabsf((3.f * z[k]) * z[k]) + fabsf((2.f * A) * z[k])) + fabsf(B));
    }
    return ok ? n : 0;
}

// the sample of hypothesis `hyp`, normalised
template <int M> __device__ __forceinline__ void tv_gather(const TvHeader& h, const f32x4* corr, unsigned seed, unsigned hyp, f32x4 (&q)[M]) {
    int pick[M];
    tv_sample<M>(seed, hyp, h.count, pick);
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const f32x4 c = corr[pick[i]];
        q[i] = f32x4{(c[0] - h.n.cx0) * h.n.s0, (c[1] - h.n.cy0) * h.n.s0, (c[2] - h.n.cx1) * h.n.s1, (c[3] - h.n.cy1) * h.n.s1};
    }
}
// the models of hypothesis `hyp` of a pair, denormalised, unit norm: m[r] valid for r < the returned number (invalid ones in between are all zero, see valid[])
template <int KIND> __device__ __forceinline__ int tv_models(const TvArgs& a, const TvHeader& h, const f32x4* corr, int pair, int hyp, float (&m)[3][9], bool (&valid)[3]) {
    valid[0] = valid[1] = valid[2] = false;
    if (a.given) {
        const float* src = a.models_in + ((long long)pair * a.hyps + hyp) * 9;
        bool any = false;
#pragma unroll
        for (int e = 0; e < 9; ++e) { m[0][e] = src[e]; m[1][e] = m[2][e] = 0.f; any = any || src[e] != 0.f; }
        valid[0] = any && tv_finite9(m[0]);
        tv_output_form(m[0]);
        return 1;
    }
    if (KIND == TV_H) {
        f32x4 q[4];
        tv_gather<4>(h, corr, a.seed, (unsigned)hyp, q);
        const bool ok = tv_solve_h(q, m[0]);
        tv_denormalise<TV_H, float>(m[0], h.n);
        valid[0] = tv_unit(m[0]) && ok;
        return 1;
    } else {
        f32x4 q[7];
        float n1[9], n2[9], z[3];
        bool well[3];
        tv_gather<7>(h, corr, a.seed, (unsigned)hyp, q);
        const int n = tv_solve_f(q, n1, n2, z, well);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int e = 0; e < 9; ++e) m[r][e] = n1[e] + z[r] * n2[e];
            tv_denormalise<TV_F, float>(m[r], h.n);
            valid[r] = tv_unit(m[r]) && well[r] && r < n;
        }
        return n > 0 ? n : 1;
    }
}

// ------------------------------------------------------------------ hypotheses: one lane each
template <int KIND> __global__ __launch_bounds__(TV_THREADS) void tv_hypothesis_kernel(TvArgs a) {
    __shared__ f32x4 tile[TV_TILE];
    const int pair = a.pair0 + blockIdx.x, tid = threadIdx.x, hyp = blockIdx.y * TV_THREADS + tid;
    const TvHeader h = a.head[pair];
    const int S = h.count;
    if (S < (a.given ? 1 : KIND == TV_H ? 4 : 7)) return;       // uniform per workgroup: the key stays 0
    const f32x4* corr = a.corr + (long long)pair * a.src.n0;
    float m[3][9]; bool valid[3];
    tv_models<KIND>(a, h, corr, pair, hyp, m, valid);
    int pos[3] = {0, 0, 0}, neg[3] = {0, 0, 0};
    tv_score_tiles<KIND, (KIND == TV_H ? 1 : 3)>(m, corr, S, a.t2, tile, pos, neg);
    unsigned key = 0u;
#pragma unroll
    for (int r = (KIND == TV_H ? 0 : 2); r >= 0; --r) {
        const int count = valid[r] ? max(pos[r], neg[r]) : 0;
        key = max(key, TvKey::make(count, hyp, r));
    }
    publish_winner(key, &a.head[pair].key);
}

// ------------------------------------------------------------------ finalise: one workgroup per pair
template <int KIND> __global__ __launch_bounds__(TV_THREADS) void tv_finalise_kernel(TvArgs a) {
    __shared__ unsigned char mask[LG_MAX_KEYPOINTS];
    __shared__ float model[2][9];
    __shared__ int red8[8], flag;
    __shared__ double red4[4], JA[81], JV[81], J3[9], V3[9];
    const int pair = a.pair0 + blockIdx.x, tid = threadIdx.x, n0 = a.src.n0;
    const bool ok = pair_images(a.src.px, pair).ok;
    const TvHeader h = a.head[pair];
    const int S = h.count;
    const long long at = (long long)pair * n0;
    const f32x4* corr = a.corr + at; const int* rows = a.rows + at;
    const unsigned key = h.key;
    const int hyp = TvKey::hyp_of(key), root = TvKey::root_of(key);
    for (int i = tid; i < n0; i += TV_THREADS) mask[i] = 0;
    float fin[9];
    TvCount cur{0, 1};
    if (key) {                                           // uniform per workgroup
        if (tid == 0) {
            float m[3][9]; bool valid[3];
            tv_models<KIND>(a, h, corr, pair, hyp, m, valid);
#pragma unroll
            for (int r = 0; r < 3; ++r) if (r == root) for (int e = 0; e < 9; ++e) model[0][e] = m[r][e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 9; ++e) fin[e] = model[0][e];
        cur = tv_count<KIND>(fin, corr, S, a.t2, red8);
        if (a.refine && cur.count >= (KIND == TV_H ? 4 : 8)) {
            double f[9];
            tv_null_vector<KIND>(fin, cur.sign, corr, S, a.t2, h.n, [](const f32x4& c) { return c; }, JA, JV, red4, f);
            if (tid == 0) {
                if (KIND == TV_F) {                      // rank 2: F - (F v3) v3^T, v3 the smallest eigenvector of F^T F
                    ata3(f, J3);
                    const int c3 = tv_jacobi(J3, V3, 3);
                    const double v3[3] = {V3[c3], V3[3 + c3], V3[6 + c3]};
                    for (int r = 0; r < 3; ++r) {
                        const double fv = f[3 * r] * v3[0] + f[3 * r + 1] * v3[1] + f[3 * r + 2] * v3[2];
                        for (int c = 0; c < 3; ++c) f[3 * r + c] -= fv * v3[c];
                    }
                }
                tv_denormalise<KIND, double>(f, h.n);
                double sq = 0;
                for (int e = 0; e < 9; ++e) sq += f[e] * f[e];
                const double nrm = sqrt(sq);
                bool good = nrm > 0 && isfinite(nrm);
                float ref[9];
                for (int e = 0; e < 9; ++e) { ref[e] = good ? (float)(f[e] / nrm) : 0.f; good = good && isfinite(ref[e]); }
                tv_output_form(ref);
                for (int e = 0; e < 9; ++e) model[1][e] = ref[e];
                flag = good ? 1 : 0;
            }
            __syncthreads();
            if (flag) tv_keep_if_not_worse<KIND>(model[1], corr, S, a.t2, red8, cur, fin);       // uniform
        }
    }
    const bool empty = !key || cur.count == 0;
    __syncthreads();                                     // mask[] is zeroed
    tv_mark_inliers<KIND>(empty, fin, cur.sign, corr, rows, S, a.t2, mask);
    __syncthreads();
    tv_write_rows(n0, mask, a.src.matches0 + at, a.inliers0 + at, a.matches0_out ? a.matches0_out + at : nullptr);
    if (tid == 0) {
        for (int e = 0; e < 9; ++e) a.models[(long long)pair * 9 + e] = empty ? 0.f : fin[e];      // in output form since it was made
        a.num_inliers[pair] = empty ? 0 : cur.count;
        if (a.best) a.best[pair] = empty ? -1 : hyp;
        a.status[pair] = ok ? LG_OK : LG_ERR_INDEX;
    }
}

// ------------------------------------------------------------------ host side
template <int KIND> static void tv_launch(const TvArgs& a, int count, hipStream_t s) {
    hipLaunchKernelGGL(tv_compact_kernel, dim3(count), dim3(TV_THREADS), 0, s, a);
    hipLaunchKernelGGL(tv_hypothesis_kernel<KIND>, dim3(count, a.hyps / TV_THREADS), dim3(TV_THREADS), 0, s, a);
    hipLaunchKernelGGL(tv_finalise_kernel<KIND>, dim3(count), dim3(TV_THREADS), 0, s, a);
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_twoview_workspace_bytes(int64_t pairs, int32_t n0, uint32_t flags) {
    TvLayout L;
    return tv_layout(pairs, n0, flags, L) ? -1 : L.total;
}

int lg_twoview_verify(const lg_twoview_io* io, void* hip_stream) {
    TvLayout L;
    if (const int rc = check_estimator_call("lg_twoview_verify", "lg_twoview_workspace_bytes", io, L)) return rc;
    const bool indexed = io->flags & LG_FLAG_INDEXED, given = io->flags & LG_TWOVIEW_GIVEN_MODELS;
    const int P = io->pairs, n0 = io->n0, n1 = io->n1;
    if (P == 0) return LG_OK;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(io->workspace);
    TvArgs a{};
    a.src.n0 = n0; a.src.n1 = n1;
    if (indexed) a.src.px = PairIndex{io->index0, io->index1, io->images0, io->images1};
    a.kind = (io->flags & LG_TWOVIEW_HOMOGRAPHY) ? TV_H : TV_F; a.refine = (io->flags & LG_TWOVIEW_REFINE) ? 1 : 0; a.given = given ? 1 : 0;
    a.hyps = io->num_hypotheses; a.seed = io->seed; a.t2 = io->threshold * io->threshold;
    a.src.kpts0 = io->kpts0; a.src.kpts1 = io->kpts1; a.src.num0 = io->num0; a.src.num1 = io->num1;
    a.src.matches0 = reinterpret_cast<const long long*>(io->matches0); a.models_in = io->models_in;
    a.head = reinterpret_cast<TvHeader*>(ws + L.head); a.corr = reinterpret_cast<f32x4*>(ws + L.corr); a.rows = reinterpret_cast<int*>(ws + L.rows);
    a.models = io->models; a.inliers0 = io->inliers0; a.num_inliers = io->num_inliers;
    a.matches0_out = reinterpret_cast<long long*>(io->matches0_out); a.best = io->best_hypothesis; a.status = io->status;
    return for_pair_launches(P, [&](int p0, int count) -> int {
        a.pair0 = p0;
        if (a.kind == TV_H) tv_launch<TV_H>(a, count, s); else tv_launch<TV_F>(a, count, s);
        HIPCHK(hipGetLastError());
        return LG_OK;
    });
}

}  // extern "C"
