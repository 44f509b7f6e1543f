// lightglue_amd — absolute pose of a query camera against a known model: P3P RANSAC with a fixed hypothesis budget over 2-D - 3-D matches, per pair or pooled
// per query (lg_abspose_estimate; the definition is in include/lightglue_amd.h).  Three launches per call:
//   ap_compact   one workgroup per problem: the verifier's ordered compaction (compact_slot) over the problem's pairs into one list of (x, y, X, Y, Z) and the
//                row's place in the problem, then the centroid (fp64, fixed block order), its subtraction, and the problem's camera, checked, into a 64-byte record;
//   ap_score     problems x (H / 256) workgroups, one LANE per hypothesis: the lane draws 3 correspondences, solves Grunert's quartic in fp64 and keeps its <= 4
//                candidates (R | t'), 48 floats, in registers; then all lanes stream the list through LDS in tiles and count inliers; the best of the problem
//                by one 64-bit atomicMax on (count, ~hypothesis, ~root).  Every per-lane array is indexed statically (profiles/absolute_pose.md has the
//                compiler's figures);
//   ap_finalise  one workgroup per problem: the winner solved again by one lane (nothing is stored per hypothesis), the optional five Gauss-Newton steps in
//                fp64, the keep-or-drop count, t' -> t, and the per-pair masks, counts and matches scattered through the rows' places.
// The sampler, the tile geometry, bearing, horner<N>, the winner's key (PoseKey, publish_winner) and
// the two-row accumulate_upper2<6> / reduce_upper<6> of the Gauss-Newton system are lg_ransac_common.h's; block_sum, compact_slot and the camera rule are
// lg_common.h's.  The refusals (check_estimator_call) and the workspace layout (ApLayout) are lg_host_call.h's.  What is the estimator's own is here: the 3-D
// list with its centroid, Grunert's solver and its unrolled degree-4 root finder, the reprojection test and its tile loop, the Gauss-Newton update and the scatter of a problem's mask to its pairs.
#include "lg_host_call.h"
#include "lg_kernels.h"
#include "lg_ransac_common.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr int AP_ROOTS = LG_ABSPOSE_ROOTS;
constexpr double AP_EPS = 1e-12;
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct ApHeader { unsigned long long key; int count, bad; float cam[4]; float c[3]; int pad[5]; };      // 64 bytes per problem
static_assert(sizeof(ApHeader) == 64, "lg_abspose_workspace_bytes counts 64 bytes");

struct ApArgs {
    int group0, pairs, n0, n1, refine, hyps, grouped;
    unsigned seed; float t2;
    PairIndex px;
    const float* kpts0; const int* num0; const int* num1; const long long* matches0;
    const float* points; const float* cameras0; const float* poses_in;
    const int* group_offsets; const int* group_pairs;
    ApHeader* head; f32x4* ca; f32x2* cb; int* rows;                         // workspace
    float* rotations; float* translations; int* num_inliers; int* best; float* cand;
    unsigned char* inliers0; int* pair_num_inliers; long long* matches0_out; int* status;
};

// the places [beg, end) of problem g in the grouped order (offsets clamped into their range), and the pair at a place (-1: not a pair of the call)
struct ApSpan { int beg, end; };
__device__ __forceinline__ ApSpan ap_span(const ApArgs& a, int g) {
    if (!a.grouped) return {g, g + 1};
    const int beg = min(max(a.group_offsets[g], 0), a.pairs);
    return {beg, min(max(a.group_offsets[g + 1], beg), a.pairs)};
}
__device__ __forceinline__ int ap_pair(const ApArgs& a, int place) {
    if (!a.grouped) return place;
    const int p = a.group_pairs[place];
    return (unsigned)p < (unsigned)a.pairs ? p : -1;
}

// ------------------------------------------------------------------ compaction: one workgroup per problem
__global__ __launch_bounds__(TV_THREADS) void ap_compact_kernel(ApArgs a) {
    __shared__ int wsum[4];
    __shared__ double red4[4];
    const int g = a.group0 + blockIdx.x, tid = threadIdx.x, n0 = a.n0;
    const ApSpan sp = ap_span(a, g);
    const long long at = (long long)sp.beg * n0;
    f32x4* ca = a.ca + at; f32x2* cb = a.cb + at; int* rows = a.rows + at;
    int base = 0, cam_image = -1;
    for (int place = sp.beg; place < sp.end; ++place) {  // everything in this loop's control is uniform per workgroup
        const int pair = ap_pair(a, place);
        if (pair < 0) continue;
        const PairImages src = pair_images(a.px, pair);
        if (!src.ok) continue;
        if (cam_image < 0) cam_image = src.i0;
        const int live0 = live_rows(a.num0, src.i0, n0), live1 = live_rows(a.num1, src.i1, a.n1);
        const long long m_at = (long long)pair * n0;
        for (int r0 = 0; r0 < live0; r0 += TV_THREADS) { // rows at or beyond num0 are unmatched and never read
            const int i = r0 + tid;
            long long m = -1;
            if (i < live0) m = a.matches0[m_at + i];
            bool take = m >= 0 && m < live1;             // live1 <= n1
            float X = 0.f, Y = 0.f, Z = 0.f;
            if (take) {
                const float* q = a.points + ((long long)src.i1 * a.n1 + m) * 3;
                X = q[0]; Y = q[1]; Z = q[2];
                take = isfinite(X) && isfinite(Y) && isfinite(Z);
            }
            const int k = compact_slot(take, base, wsum);
            if (take) {
                const float* p0 = a.kpts0 + ((long long)src.i0 * n0 + i) * 2;
                ca[k] = f32x4{p0[0], p0[1], X, Y};
                cb[k] = f32x2{Z, 0.f};
                rows[k] = (place - sp.beg) * n0 + i;
            }
        }
    }
    const int S = base;
    __syncthreads();                                     // the list is complete and visible to the workgroup
    double sx = 0, sy = 0, sz = 0;
    for (int k = tid; k < S; k += TV_THREADS) { const f32x4 c = ca[k]; sx += c[2]; sy += c[3]; sz += cb[k][0]; }
    const double inv = S ? 1.0 / S : 0.0;
    const float c0 = (float)(block_sum(sx, red4) * inv), c1 = (float)(block_sum(sy, red4) * inv), c2 = (float)(block_sum(sz, red4) * inv);
    for (int k = tid; k < S; k += TV_THREADS) {
        f32x4 c = ca[k]; f32x2 d = cb[k];
        c[2] = c[2] - c0; c[3] = c[3] - c1; d[0] = d[0] - c2;
        ca[k] = c; cb[k] = d;
    }
    if (tid == 0) {
        ApHeader h{};
        h.count = S; h.c[0] = c0; h.c[1] = c1; h.c[2] = c2;
        if (cam_image >= 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) h.cam[e] = a.cameras0[(long long)cam_image * 4 + e];
            h.bad = camera_ok(h.cam) ? 0 : 1;
        }
        if (h.bad) h.count = 0;                          // an empty problem to every later launch
        a.head[g] = h;
    }
}

// ------------------------------------------------------------------ the P3P solver, fp64, one lane, every array indexed statically
// the real roots of p (degree N, p[N] != 0) in ascending order, the rest of root[] zero: lg_relpose.hip's rp_real_roots (the roots of the k-th derivative lie one in each
// interval between those of the (k + 1)-th; 64 bisections and 3 guarded Newton steps per sign change; every derivative padded with zeros to degree N, which changes no
// bit), unrolled so that no index is a run-time value and nothing goes to scratch
template <int N> __device__ __forceinline__ int ap_real_roots(const double (&p)[N + 1], double (&root)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) root[i] = 0.0;
    if (!(fabs(p[N]) > 0.0)) return 0;
    double bound = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) bound = fmax(bound, fabs(p[i] / p[N]));
    bound = bound + 1.0;                                 // Cauchy; the roots of every derivative lie inside it too (Gauss-Lucas)
    if (!isfinite(bound)) return 0;
    int nprev = 0;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        double c[N + 1], dc[N + 1], nxt[N];
#pragma unroll
        for (int i = 0; i <= N; ++i) {
            double f = 0.0;
            if (i + k <= N) {
                f = p[i + k];
#pragma unroll
                for (int j = 1; j <= k; ++j) f = f * (double)(i + j);
            }
            c[i] = f;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) { dc[i] = c[i + 1] * (double)(i + 1); nxt[i] = 0.0; }
        dc[N] = 0.0;
        int n = 0;
        double lo = -bound, flo = horner<N>(c, lo);
#pragma unroll
        for (int s = 0; s < N - k; ++s) {                // the derivative above has at most N - k - 1 roots: at most N - k intervals
            if (s <= nprev) {
                const double hi = s < nprev ? root[s] : bound, fhi = horner<N>(c, hi);
                if ((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0)) {
                    double x0 = lo, x1 = hi;
#pragma unroll 1
                    for (int it = 0; it < 64; ++it) {
                        const double m = 0.5 * (x0 + x1), fm = horner<N>(c, m);
                        if ((fm < 0.0) == (flo < 0.0)) x0 = m; else x1 = m;
                    }
                    double z = 0.5 * (x0 + x1);
#pragma unroll 1
                    for (int it = 0; it < 3; ++it) {
                        const double zn = z - horner<N>(c, z) / horner<N>(dc, z);
                        if (zn >= x0 && zn <= x1) z = zn;
                    }
#pragma unroll
                    for (int e = 0; e < N; ++e) nxt[e] = e == n ? z : nxt[e];
                    ++n;
                }
                lo = hi; flo = fhi;
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) root[i] = nxt[i];
        nprev = n;
    }
    return nprev;
}

__device__ __forceinline__ void ap_cross(const double (&u)[3], const double (&v)[3], double (&w)[3]) {
    w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ __forceinline__ double ap_dot(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// e1 = (B - A) / |.|, e3 = e1 x (C - A) normalised, e2 = e3 x e1
__device__ __forceinline__ void ap_frame(const double (&A)[3], const double (&B)[3], const double (&C)[3], double (&e1)[3], double (&e2)[3], double (&e3)[3]) {
    double d[3], f[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) { d[e] = B[e] - A[e]; f[e] = C[e] - A[e]; }
    const double n1 = sqrt(ap_dot(d, d));
#pragma unroll
    for (int e = 0; e < 3; ++e) e1[e] = d[e] / n1;
    ap_cross(e1, f, e3);
    const double n3 = sqrt(ap_dot(e3, e3));
#pragma unroll
    for (int e = 0; e < 3; ++e) e3[e] = e3[e] / n3;
    ap_cross(e3, e1, e2);
}

// the candidates (R | t') of three correspondences q[k] = (x, y, X', Y', Z'), root index ascending in v; an invalid slot is all zero
__device__ __forceinline__ void ap_p3p(const float (&q)[3][5], const float (&cam)[4], float (&cand)[AP_ROOTS][12]) {
    double f[3][3], P[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double bx = (double)bearing(q[k][0], cam[2], cam[0]), by = (double)bearing(q[k][1], cam[3], cam[1]);
        const double n = sqrt((bx * bx + by * by) + 1.0);
        f[k][0] = bx / n; f[k][1] = by / n; f[k][2] = 1.0 / n;
#pragma unroll
        for (int e = 0; e < 3; ++e) P[k][e] = (double)q[k][2 + e];
    }
    double d23[3], d13[3], d12[3], d21[3], d31[3], nrm[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) { d23[e] = P[1][e] - P[2][e]; d13[e] = P[0][e] - P[2][e]; d12[e] = P[0][e] - P[1][e]; d21[e] = P[1][e] - P[0][e]; d31[e] = P[2][e] - P[0][e]; }
    const double a2 = ap_dot(d23, d23), b2 = ap_dot(d13, d13), c2 = ap_dot(d12, d12);
    ap_cross(d21, d31, nrm);
    const double ca = ap_dot(f[1], f[2]), cb = ap_dot(f[0], f[2]), cg = ap_dot(f[0], f[1]);
    const double k = (a2 - c2) / b2, m = (a2 + c2) / b2, cb2 = c2 / b2, ab2 = a2 / b2;
    double p[5];
    p[4] = (k - 1.0) * (k - 1.0) - 4.0 * cb2 * (ca * ca);
    p[3] = 4.0 * ((k * (1.0 - k) * cb - (1.0 - m) * ca * cg) + 2.0 * cb2 * (ca * ca) * cb);
    p[2] = 2.0 * (((((k * k - 1.0) + 2.0 * (k * k) * (cb * cb)) + 2.0 * ((b2 - c2) / b2) * (ca * ca)) - 4.0 * m * ca * cb * cg) + 2.0 * ((b2 - a2) / b2) * (cg * cg));
    p[1] = 4.0 * ((-k * (1.0 + k) * cb + 2.0 * ab2 * (cg * cg) * cb) - (1.0 - m) * ca * cg);
    p[0] = (1.0 + k) * (1.0 + k) - 4.0 * ab2 * (cg * cg);
    bool ok = b2 > 0.0 && sqrt(ap_dot(nrm, nrm)) > AP_EPS * (sqrt(b2) * sqrt(c2));
#pragma unroll
    for (int e = 0; e < 5; ++e) ok = ok && isfinite(p[e]);
    double root[4] = {0.0, 0.0, 0.0, 0.0};
    int n = 0;
    if (ok) n = ap_real_roots<4>(p, root);
    double w1[3], w2[3], w3[3], mp[3];
    ap_frame(P[0], P[1], P[2], w1, w2, w3);
#pragma unroll
    for (int e = 0; e < 3; ++e) mp[e] = ((P[0][e] + P[1][e]) + P[2][e]) / 3.0;
#pragma unroll
    for (int r = 0; r < AP_ROOTS; ++r) {
        const double v = root[r], den = cg - v * ca;
        const double u = (((k - 1.0) * (v * v) - 2.0 * k * cb * v) + (1.0 + k)) / (2.0 * den);
        const double q1 = (1.0 + u * u) - 2.0 * u * cg;
        bool good = ok && r < n && v > 0.0 && fabs(den) > AP_EPS && u > 0.0 && q1 > 0.0;
        const double s1 = sqrt(c2 / q1), s2 = u * s1, s3 = v * s1;
        double C0[3], C1[3], C2[3], e1[3], e2[3], e3[3], mc[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) { C0[e] = s1 * f[0][e]; C1[e] = s2 * f[1][e]; C2[e] = s3 * f[2][e]; mc[e] = ((C0[e] + C1[e]) + C2[e]) / 3.0; }
        ap_frame(C0, C1, C2, e1, e2, e3);
        float out[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double R[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { R[j] = (e1[i] * w1[j] + e2[i] * w2[j]) + e3[i] * w3[j]; out[4 * i + j] = (float)R[j]; }
            const double t = mc[i] - ap_dot(R, mp);
            out[4 * i + 3] = (float)t;
            good = good && isfinite(R[0]) && isfinite(R[1]) && isfinite(R[2]) && isfinite(t);
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) good = good && isfinite(out[e]);
#pragma unroll
        for (int e = 0; e < 12; ++e) cand[r][e] = good ? out[e] : 0.f;
    }
}

// t' = t + R c (LG_ABSPOSE_GIVEN_POSES, and the re-centring of a returned pose): fp64, rounded to float32; all zero if anything is non-finite or the pose is all zero
__device__ __forceinline__ void ap_centre(const float (&pose)[12], const float (&c)[3], float (&m)[12]) {
    bool any = false, fin = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) { any = any || pose[e] != 0.f; fin = fin && isfinite(pose[e]); m[e] = pose[e]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        m[4 * i + 3] = (float)((double)pose[4 * i + 3] + (((double)pose[4 * i] * (double)c[0] + (double)pose[4 * i + 1] * (double)c[1]) + (double)pose[4 * i + 2] * (double)c[2]));
        fin = fin && isfinite(m[4 * i + 3]);
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) m[e] = any && fin ? m[e] : 0.f;
}
// t = t' - R c: fp64, rounded to float32
__device__ __forceinline__ float ap_world_t(const float (&m)[12], const float (&c)[3], int i) {
    return (float)((double)m[4 * i + 3] - (((double)m[4 * i] * (double)c[0] + (double)m[4 * i + 1] * (double)c[1]) + (double)m[4 * i + 2] * (double)c[2]));
}

// the candidates of hypothesis `hyp` of a problem: its sample solved, or the given pose re-centred (R = 1 candidate).  S >= 3 (GIVEN: nothing is sampled)
template <bool GIVEN, int R> __device__ __forceinline__ void ap_hypothesis(const ApArgs& a, const ApHeader& h, int g, int hyp, const f32x4* ca, const f32x2* cb, float (&m)[R][12]) {
    if (GIVEN) {
        const float* src = a.poses_in + ((long long)g * a.hyps + hyp) * 12;
        float pose[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) pose[e] = src[e];
        ap_centre(pose, h.c, m[0]);
    } else {
        int pick[3];
        tv_sample<3>(a.seed, (unsigned)hyp, h.count, pick);
        float q[3][5];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const f32x4 c = ca[pick[k]];
            q[k][0] = c[0]; q[k][1] = c[1]; q[k][2] = c[2]; q[k][3] = c[3]; q[k][4] = cb[pick[k]][0];
        }
        float full[AP_ROOTS][12];
        ap_p3p(q, h.cam, full);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 12; ++e) m[r][e] = full[r][e];
    }
}

// ------------------------------------------------------------------ the inlier test
__device__ __forceinline__ bool ap_test(const float (&m)[12], const f32x4& p, float Z, const float (&cam)[4], float t2) {
    const float x = p[0], y = p[1], X = p[2], Y = p[3];
    const float px = fmaf(m[0], X, fmaf(m[1], Y, fmaf(m[2], Z, m[3]))), py = fmaf(m[4], X, fmaf(m[5], Y, fmaf(m[6], Z, m[7])));
    const float pz = fmaf(m[8], X, fmaf(m[9], Y, fmaf(m[10], Z, m[11])));
    const float ex = fmaf(cam[0], px, (cam[2] - x) * pz), ey = fmaf(cam[1], py, (cam[3] - y) * pz);
    return pz > 0.f && fmaf(ex, ex, ey * ey) <= t2 * (pz * pz);
}

// ------------------------------------------------------------------ solve + score: one lane per hypothesis
template <bool GIVEN> __global__ __launch_bounds__(TV_THREADS) void ap_score_kernel(ApArgs a) {
    constexpr int R = GIVEN ? 1 : AP_ROOTS;
    __shared__ f32x4 ta[TV_TILE];
    __shared__ f32x2 tb[TV_TILE];
    const int g = a.group0 + blockIdx.x, tid = threadIdx.x, hyp = blockIdx.y * TV_THREADS + tid;
    const ApHeader h = a.head[g];
    const int S = h.count;
    const long long at = (long long)ap_span(a, g).beg * a.n0;
    const f32x4* ca = a.ca + at; const f32x2* cb = a.cb + at;
    float m[R][12];
    if (S >= (GIVEN ? 1 : 3)) ap_hypothesis<GIVEN, R>(a, h, g, hyp, ca, cb, m);      // uniform per workgroup
    else {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 12; ++e) m[r][e] = 0.f;
    }
    if (!GIVEN && a.cand) {
        float* out = a.cand + ((long long)g * a.hyps + hyp) * (AP_ROOTS * 12);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < 12; ++e) out[r * 12 + e] = (e & 3) == 3 ? ap_world_t(m[r], h.c, e >> 2) : m[r][e];
    }
    if (S < (GIVEN ? 1 : 3)) return;                     // the key stays 0
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) cnt[r] = 0;
    for (int t0 = 0; t0 < S; t0 += TV_TILE) {
        if (t0) __syncthreads();
        if (t0 + tid < S) { ta[tid] = ca[t0 + tid]; tb[tid] = cb[t0 + tid]; }
        __syncthreads();
        const int n = min(TV_TILE, S - t0);
        for (int j = 0; j < n; ++j) {
            const f32x4 p = ta[j];                       // one address for the whole wave: a broadcast
            const float Z = tb[j][0];
#pragma unroll
            for (int r = 0; r < R; ++r) cnt[r] += ap_test(m[r], p, Z, h.cam, a.t2) ? 1 : 0;
        }
    }
    unsigned long long key = 0ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned long long kr = PoseKey::make(cnt[r], hyp, r);
        key = kr > key ? kr : key;
    }
    publish_winner(key, &a.head[g].key);
}

// ------------------------------------------------------------------ finalise: one workgroup per problem
// the inlier count of candidate m over the problem's list, the same number in every thread
__device__ __forceinline__ int ap_count(const float (&m)[12], const f32x4* ca, const f32x2* cb, int S, const float (&cam)[4], float t2, int* red4i) {
    int cnt = 0;
    for (int k = threadIdx.x; k < S; k += TV_THREADS) cnt += ap_test(m, ca[k], cb[k][0], cam, t2) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4i[threadIdx.x >> 6] = cnt;
    __syncthreads();
    return ((red4i[0] + red4i[1]) + red4i[2]) + red4i[3];
}
// one Gauss-Newton step by one lane: A [6][7] = (J^T J | -J^T r), solved by Gaussian elimination with row pivoting; pose [12] (R | t') <- the update.  false: abandoned
__device__ bool ap_gn_update(double* A, double* pose) {
    double big = 0.0;
    for (int i = 0; i < 6; ++i) big = fmax(big, A[i * 7 + i]);
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        for (int i = k + 1; i < 6; ++i) if (fabs(A[i * 7 + k]) > fabs(A[piv * 7 + k])) piv = i;
        if (piv != k) for (int c = k; c < 7; ++c) { const double t = A[k * 7 + c]; A[k * 7 + c] = A[piv * 7 + c]; A[piv * 7 + c] = t; }
        const double p = A[k * 7 + k];
        if (!(fabs(p) > AP_EPS * big)) return false;
        for (int i = k + 1; i < 6; ++i) {
            const double f = A[i * 7 + k] / p;
            for (int c = k; c < 7; ++c) A[i * 7 + c] = A[i * 7 + c] - f * A[k * 7 + c];
        }
    }
    double x[6];
    for (int k = 5; k >= 0; --k) {
        double s = A[k * 7 + 6];
        for (int c = k + 1; c < 6; ++c) s = s - A[k * 7 + c] * x[c];
        x[k] = s / A[k * 7 + k];
    }
    // Rodrigues(w) = I + sin(th) [k]x + (1 - cos(th)) [k]x^2, k = w / th
    const double th = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    double Q[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (th > 0.0) {
        const double kx = x[0] / th, ky = x[1] / th, kz = x[2] / th, s = sin(th), c1 = 1.0 - cos(th);
        const double K[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
                Q[3 * i + j] = (Q[3 * i + j] + s * K[3 * i + j]) + c1 * kk;
            }
    }
    double out[12];
    bool fin = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            out[4 * i + j] = ((Q[3 * i] * pose[j] + Q[3 * i + 1] * pose[4 + j]) + Q[3 * i + 2] * pose[8 + j]) + (j == 3 ? x[3 + i] : 0.0);
            fin = fin && isfinite(out[4 * i + j]);
        }
    if (!fin) return false;
    for (int e = 0; e < 12; ++e) pose[e] = out[e];
    return true;
}

template <bool GIVEN> __global__ __launch_bounds__(TV_THREADS) void ap_finalise_kernel(ApArgs a) {
    constexpr int R = GIVEN ? 1 : AP_ROOTS;
    __shared__ float win[12];
    __shared__ int red4i[4], flag;
    __shared__ double red4[4], A[42], pose[12];
    const int g = a.group0 + blockIdx.x, tid = threadIdx.x, n0 = a.n0;
    const ApSpan sp = ap_span(a, g);
    const ApHeader h = a.head[g];
    const int S = h.count;
    const long long at = (long long)sp.beg * n0;
    const f32x4* ca = a.ca + at; const f32x2* cb = a.cb + at; const int* rows = a.rows + at;
    const unsigned long long key = h.key;
    const int hyp = PoseKey::hyp_of(key), root = PoseKey::root_of(key);
    // every pair of the problem: its status, an all-false mask, no match, no inlier
    for (int place = sp.beg; place < sp.end; ++place) {
        const int pair = ap_pair(a, place);
        if (pair < 0) continue;
        const long long m_at = (long long)pair * n0;
        for (int i = tid; i < n0; i += TV_THREADS) {
            a.inliers0[m_at + i] = 0;
            if (a.matches0_out) a.matches0_out[m_at + i] = -1;
        }
        if (tid == 0) {
            a.pair_num_inliers[pair] = 0;
            a.status[pair] = !pair_images(a.px, pair).ok ? LG_ERR_INDEX : h.bad ? LG_ERR_CAMERA : LG_OK;
        }
    }
    float fin[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) fin[e] = 0.f;
    int cur = 0;
    if (key) {                                           // uniform per workgroup
        if (tid == 0) {
            float m[R][12];
            ap_hypothesis<GIVEN, R>(a, h, g, hyp, ca, cb, m);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r == root)
#pragma unroll
                    for (int e = 0; e < 12; ++e) win[e] = m[r][e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 12; ++e) fin[e] = win[e];
        cur = ap_count(fin, ca, cb, S, h.cam, a.t2, red4i);
        if (a.refine && cur >= 4) {
            const double fx = h.cam[0], fy = h.cam[1], cx = h.cam[2], cy = h.cam[3];
            if (tid == 0) { for (int e = 0; e < 12; ++e) pose[e] = (double)fin[e]; flag = 1; }
            __syncthreads();
#pragma unroll 1
            for (int step = 0; step < 5; ++step) {
                double P[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) P[e] = pose[e];
                double acc[21], rhs[6];                 // the upper triangle of J^T J, and J^T r
#pragma unroll
                for (int e = 0; e < 21; ++e) acc[e] = 0.0;
#pragma unroll
                for (int e = 0; e < 6; ++e) rhs[e] = 0.0;
                for (int k = tid; k < S; k += TV_THREADS) {
                    const f32x4 c = ca[k];
                    const float Zf = cb[k][0];
                    if (!ap_test(fin, c, Zf, h.cam, a.t2)) continue;        // the winner's inlier set
                    const double X = c[2], Y = c[3], Z = Zf;
                    const double px = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3], py = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7], pz = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
                    if (!(pz > 0.0)) continue;
                    const double iz = 1.0 / pz, ja = fx * iz, jb = -(fx * px) * (iz * iz), jc = fy * iz, jd = -(fy * py) * (iz * iz);
                    const double r0 = (fx * px * iz + cx) - (double)c[0], r1 = (fy * py * iz + cy) - (double)c[1];
                    const double J0[6] = {jb * py, ja * pz - jb * px, -(ja * py), ja, 0.0, jb};
                    const double J1[6] = {jd * py - jc * pz, -(jd * px), jc * px, 0.0, jc, jd};
                    accumulate_upper2<6>(acc, J0, J1);
#pragma unroll
                    for (int p = 0; p < 6; ++p) rhs[p] += J0[p] * r0 + J1[p] * r1;
                }
                reduce_upper<6>(acc, A, 7, red4);
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    const double s = block_sum(rhs[p], red4);
                    if (tid == 0) A[p * 7 + 6] = -s;
                }
                if (tid == 0) flag = ap_gn_update(A, pose) ? 1 : 0;
                __syncthreads();
                if (!flag) break;                        // uniform
            }
            if (flag) {
                float ref[12];
                bool good = true;
#pragma unroll
                for (int e = 0; e < 12; ++e) { ref[e] = (float)pose[e]; good = good && isfinite(ref[e]); }
                if (good) {                              // uniform: every thread read the same pose
                    const int again = ap_count(ref, ca, cb, S, h.cam, a.t2, red4i);
                    if (again >= cur) {
                        cur = again;
#pragma unroll
                        for (int e = 0; e < 12; ++e) fin[e] = ref[e];
                    }
                }
            }
        }
    }
    // the returned pose in the world frame, and its own mask: re-centred as a given pose is
    float world[12], back[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) world[e] = (e & 3) == 3 ? ap_world_t(fin, h.c, e >> 2) : fin[e];
    ap_centre(world, h.c, back);
    int count = 0;
    if (key && cur > 0) count = ap_count(back, ca, cb, S, h.cam, a.t2, red4i);
    const bool empty = count == 0;
    __syncthreads();                                     // the cleared masks and counts are behind every thread
    if (!empty)
        for (int k = tid; k < S; k += TV_THREADS)
            if (ap_test(back, ca[k], cb[k][0], h.cam, a.t2)) {
                const int rel = rows[k], place = rel / n0, i = rel - place * n0;
                const int pair = ap_pair(a, sp.beg + place);
                const long long flat = (long long)pair * n0 + i;
                a.inliers0[flat] = 1;
                if (a.matches0_out) a.matches0_out[flat] = a.matches0[flat];
                atomicAdd(&a.pair_num_inliers[pair], 1);
            }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) a.rotations[(long long)g * 9 + 3 * i + j] = empty ? 0.f : world[4 * i + j];
            a.translations[(long long)g * 3 + i] = empty ? 0.f : world[4 * i + 3];
        }
        a.num_inliers[g] = count;
        if (a.best) a.best[g] = empty ? -1 : hyp;
    }
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_abspose_workspace_bytes(int64_t pairs, int32_t n0, int32_t num_hypotheses, uint32_t flags) {
    ApLayout L;
    return ap_layout(pairs, n0, num_hypotheses, flags, L) ? -1 : L.total;
}

int lg_abspose_estimate(const lg_abspose_io* io, void* hip_stream) {
    ApLayout L;
    if (const int rc = check_estimator_call("lg_abspose_estimate", "lg_abspose_workspace_bytes", io, L)) return rc;
    const bool indexed = io->flags & LG_FLAG_INDEXED, grouped = io->flags & LG_ABSPOSE_GROUPED, given = io->flags & LG_ABSPOSE_GIVEN_POSES;
    const int P = io->pairs, n0 = io->n0, n1 = io->n1;
    if (P == 0) return LG_OK;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(io->workspace);
    ApArgs a{};
    a.pairs = P; a.n0 = n0; a.n1 = n1; a.grouped = grouped ? 1 : 0;
    if (indexed) a.px = PairIndex{io->index0, io->index1, io->images0, io->images1};
    a.refine = (io->flags & LG_ABSPOSE_REFINE) ? 1 : 0;
    a.hyps = io->num_hypotheses; a.seed = io->seed; a.t2 = io->threshold * io->threshold;
    a.kpts0 = io->kpts0; a.num0 = io->num0; a.num1 = io->num1; a.matches0 = reinterpret_cast<const long long*>(io->matches0);
    a.points = io->points3d1; a.cameras0 = io->cameras0; a.poses_in = io->poses_in;
    a.group_offsets = io->group_offsets; a.group_pairs = io->group_pairs;
    a.head = reinterpret_cast<ApHeader*>(ws + L.head); a.ca = reinterpret_cast<f32x4*>(ws + L.ca); a.cb = reinterpret_cast<f32x2*>(ws + L.cb);
    a.rows = reinterpret_cast<int*>(ws + L.rows);
    a.rotations = io->rotations; a.translations = io->translations; a.num_inliers = io->num_inliers; a.best = io->best_hypothesis; a.cand = io->candidates;
    a.inliers0 = io->inliers0; a.pair_num_inliers = io->pair_num_inliers; a.matches0_out = reinterpret_cast<long long*>(io->matches0_out); a.status = io->status;
    return for_pair_launches(grouped ? io->groups : P, [&](int g0, int count) -> int {
        a.group0 = g0;
        hipLaunchKernelGGL(ap_compact_kernel, dim3(count), dim3(TV_THREADS), 0, s, a);
        if (given) {
            hipLaunchKernelGGL(ap_score_kernel<true>, dim3(count, a.hyps / TV_THREADS), dim3(TV_THREADS), 0, s, a);
            hipLaunchKernelGGL(ap_finalise_kernel<true>, dim3(count), dim3(TV_THREADS), 0, s, a);
        } else {
            hipLaunchKernelGGL(ap_score_kernel<false>, dim3(count, a.hyps / TV_THREADS), dim3(TV_THREADS), 0, s, a);
            hipLaunchKernelGGL(ap_finalise_kernel<false>, dim3(count), dim3(TV_THREADS), 0, s, a);
        }
        HIPCHK(hipGetLastError());
        return LG_OK;
    });
}

}  // extern "C"
