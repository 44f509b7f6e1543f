// lightglue_amd — the device code the two-view verifier (lg_twoview.hip) and the relative-pose estimator (lg_relpose.hip) share, written once: the compaction of
// matches0 into a pair's correspondence list, the counter-based sampling hash, the 9-float model helpers (output form, unit norm, denormalisation), the
// division-free inlier test, the broadcast-tile scoring loop, the workgroup inlier count and the single-lane fp64 Jacobi.  Everything here is compiled without
// floating-point contraction (the pragma below governs the rest of the including translation unit) and the inlier test is written in explicit fmaf: a model and
// a decision are the same bits in every kernel of either file.
#pragma once

#include "lg_kernels.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr int TV_THREADS = 256, TV_TILE = LG_TWOVIEW_TILE;
constexpr int TV_H = 0, TV_F = 1;                        // model kinds
static_assert(TV_TILE == TV_THREADS, "a tile is loaded by one float4 per thread");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct TvHeader { int count; unsigned key; float cx0, cy0, s0, cx1, cy1, s1; };       // 32 bytes per pair
static_assert(sizeof(TvHeader) == 32, "lg_twoview_workspace_bytes counts 32 bytes");

// what the compaction of one pair reads
struct TvSource {
    int n0, n1;
    PairIndex px;                                        // the images pair p reads (lg_common.h)
    const float* kpts0; const float* kpts1; const int* num0; const int* num1;
    const long long* matches0;
};

// ------------------------------------------------------------------ compaction: one workgroup per pair; the pair's record (key 0) comes back in every thread
__device__ __forceinline__ TvHeader tv_compact_pair(const TvSource& a, int pair, f32x4* corr, int* rows, int* wsum, double* red4) {
    const int tid = threadIdx.x;
    const PairImages src = pair_images(a.px, pair);
    const int i0 = src.i0, i1 = src.i1, live0 = src.ok ? live_rows(a.num0, i0, a.n0) : 0, live1 = src.ok ? live_rows(a.num1, i1, a.n1) : 0;
    const long long at = (long long)pair * a.n0;
    int base = 0;
    for (int r0 = 0; r0 < live0; r0 += TV_THREADS) {     // rows at or beyond num0 are unmatched and never read
        const int i = r0 + tid;
        long long m = -1;
        if (i < live0) m = a.matches0[at + i];
        const bool take = m >= 0 && m < live1;           // live1 <= n1
        const int k = compact_slot(take, base, wsum);
        if (take) {
            const float* p0 = a.kpts0 + ((long long)i0 * a.n0 + i) * 2;
            const float* p1 = a.kpts1 + ((long long)i1 * a.n1 + m) * 2;
            corr[k] = f32x4{p0[0], p0[1], p1[0], p1[1]};
            rows[k] = i;
        }
    }
    const int S = base;
    __syncthreads();                                     // the list is complete and visible to the workgroup
    // Hartley normalisation of either side, sums in fp64 (per-thread strided partial sums, then block_sum)
    double sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;
    for (int k = tid; k < S; k += TV_THREADS) { const f32x4 c = corr[k]; sx0 += c[0]; sy0 += c[1]; sx1 += c[2]; sy1 += c[3]; }
    const double inv = S ? 1.0 / S : 0.0;
    const double cx0 = block_sum(sx0, red4) * inv, cy0 = block_sum(sy0, red4) * inv;
    const double cx1 = block_sum(sx1, red4) * inv, cy1 = block_sum(sy1, red4) * inv;
    double d0 = 0, d1 = 0;
    for (int k = tid; k < S; k += TV_THREADS) {
        const f32x4 c = corr[k];
        const double ax = c[0] - cx0, ay = c[1] - cy0, bx = c[2] - cx1, by = c[3] - cy1;
        d0 += sqrt(ax * ax + ay * ay); d1 += sqrt(bx * bx + by * by);
    }
    const double m0 = block_sum(d0, red4) * inv, m1 = block_sum(d1, red4) * inv;
    TvHeader h;
    h.count = S; h.key = 0u;
    h.cx0 = (float)cx0; h.cy0 = (float)cy0; h.s0 = m0 > 0 ? (float)(1.4142135623730951 / m0) : 1.f;
    h.cx1 = (float)cx1; h.cy1 = (float)cy1; h.s1 = m1 > 0 ? (float)(1.4142135623730951 / m1) : 1.f;
    return h;
}

// ------------------------------------------------------------------ sampling
__device__ __forceinline__ unsigned tv_mix(unsigned x) { x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16; return x; }
__device__ __forceinline__ unsigned tv_hash(unsigned seed, unsigned hyp, unsigned slot) {
    return tv_mix(tv_mix(seed + 0x9E3779B9u * (hyp + 1u)) + 0x85EBCA6Bu * (slot + 1u));
}
// M distinct indices below S (S >= M): slot s draws from S - s and skips past the earlier picks, kept sorted in srt
template <int M> __device__ __forceinline__ void tv_sample(unsigned seed, unsigned hyp, int S, int (&pick)[M]) {
    int srt[M];
#pragma unroll
    for (int s = 0; s < M; ++s) {
        int d = (int)(tv_hash(seed, hyp, (unsigned)s) % (unsigned)(S - s));
#pragma unroll
        for (int e = 0; e < M; ++e) if (e < s && d >= srt[e]) ++d;
        pick[s] = d;
        int v = d;
#pragma unroll
        for (int e = 0; e < M; ++e) if (e < s) { const int lo = min(srt[e], v), hi = max(srt[e], v); srt[e] = lo; v = hi; }
        srt[s] = v;
    }
}

// ------------------------------------------------------------------ models: 9 floats, row-major
__device__ __forceinline__ bool tv_finite9(const float (&m)[9]) {
    bool f = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) f = f && isfinite(m[i]);
    return f;
}
// output form: the entry of largest magnitude (the first one among equals) positive.  Every model is scored in this form, so that "+H" means one matrix
__device__ __forceinline__ void tv_output_form(float (&m)[9]) {
    float big = m[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) big = fabsf(m[i]) > fabsf(big) ? m[i] : big;
    const float sgn = big < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = sgn * m[i];
}
// m / |m|_F in output form; false if the norm is 0 or anything is non-finite (m is then all zero)
__device__ __forceinline__ bool tv_unit(float (&m)[9]) {
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) sq = sq + m[i] * m[i];
    const float nrm = sqrtf(sq);
    bool ok = nrm > 0.f && isfinite(nrm);
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = m[i] / nrm;
    ok = ok && tv_finite9(m);
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = ok ? m[i] : 0.f;
    tv_output_form(m);
    return ok;
}
// G = M T0, T0 = [s0 0 -s0 cx0; 0 s0 -s0 cy0; 0 0 1]: the part of the denormalisation both models share
template <class T> __device__ __forceinline__ void tv_right_t0(T (&m)[9], T s0, T cx0, T cy0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const T a = m[3 * r] * s0, b = m[3 * r + 1] * s0;
        m[3 * r + 2] = (m[3 * r + 2] - a * cx0) - b * cy0;
        m[3 * r] = a; m[3 * r + 1] = b;
    }
}
// H = T1^-1 Hn T0, F = T1^T Fn T0 (T of side 1 alike)
template <int KIND, class T> __device__ __forceinline__ void tv_denormalise(T (&m)[9], T cx0, T cy0, T s0, T cx1, T cy1, T s1) {
    tv_right_t0(m, s0, cx0, cy0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (KIND == TV_H) {
            m[c] = m[c] / s1 + cx1 * m[6 + c];
            m[3 + c] = m[3 + c] / s1 + cy1 * m[6 + c];
        } else {
            const T a = m[c] * s1, b = m[3 + c] * s1;
            m[6 + c] = (m[6 + c] - a * cx1) - b * cy1;
            m[c] = a; m[3 + c] = b;
        }
    }
}

// ------------------------------------------------------------------ the inlier test: 0 = outside, +1 = inside (H: with w > 0), -1 = inside with w < 0 (H only)
template <int KIND> __device__ __forceinline__ int tv_test(const float (&m)[9], const f32x4& p, float t2) {
    const float x = p[0], y = p[1], u = p[2], v = p[3];
    const float l0 = fmaf(m[0], x, fmaf(m[1], y, m[2])), l1 = fmaf(m[3], x, fmaf(m[4], y, m[5])), l2 = fmaf(m[6], x, fmaf(m[7], y, m[8]));
    if (KIND == TV_H) {
        const float dx = fmaf(u, l2, -l0), dy = fmaf(v, l2, -l1);
        const bool in = fmaf(dx, dx, dy * dy) <= t2 * (l2 * l2);
        return in ? (l2 > 0.f ? 1 : l2 < 0.f ? -1 : 0) : 0;
    } else {
        const float r = fmaf(u, l0, fmaf(v, l1, l2));
        const float g0 = fmaf(m[0], u, fmaf(m[3], v, m[6])), g1 = fmaf(m[1], u, fmaf(m[4], v, m[7]));
        const float den = fmaf(l0, l0, fmaf(l1, l1, fmaf(g0, g0, g1 * g1)));
        return r * r <= t2 * den ? 1 : 0;
    }
}

// ------------------------------------------------------------------ scoring: every lane of the workgroup holds R models of its own and all of them see the pair's
// S correspondences, streamed through LDS in tiles of TV_TILE (tile: __shared__ f32x4[TV_TILE]); pos / neg: the inliers of either sign of the first R models.  Every thread calls
template <int KIND, int R, int RM> __device__ __forceinline__ void tv_score_tiles(const float (&m)[RM][9], const f32x4* corr, int S, float t2, f32x4* tile, int (&pos)[RM], int (&neg)[RM]) {
    const int tid = threadIdx.x;
    for (int t0 = 0; t0 < S; t0 += TV_TILE) {
        if (t0) __syncthreads();
        if (t0 + tid < S) tile[tid] = corr[t0 + tid];
        __syncthreads();
        const int cnt = min(TV_TILE, S - t0);
        for (int j = 0; j < cnt; ++j) {
            const f32x4 p = tile[j];                     // one address for the whole wave: a broadcast
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int in = tv_test<KIND>(m[r], p, t2);
                pos[r] += in > 0; neg[r] += in < 0;
            }
        }
    }
}

// ------------------------------------------------------------------ finalise: one workgroup per pair
// cyclic Jacobi on the symmetric n x n matrix A (row-major, destroyed), eigenvectors in the columns of V; returns the index of the smallest eigenvalue.  One lane.
__device__ inline int tv_jacobi(double* A, double* V, int n) {
    for (int i = 0; i < n * n; ++i) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0, diag = 0;
        for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) { const double v = A[p * n + q]; if (p == q) diag += v * v; else off += v * v; }
        if (off <= 1e-32 * diag) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) { const double x = A[k * n + p], y = A[k * n + q]; A[k * n + p] = c * x - s * y; A[k * n + q] = s * x + c * y; }
                for (int k = 0; k < n; ++k) { const double x = A[p * n + k], y = A[q * n + k]; A[p * n + k] = c * x - s * y; A[q * n + k] = s * x + c * y; }
                for (int k = 0; k < n; ++k) { const double x = V[k * n + p], y = V[k * n + q]; V[k * n + p] = c * x - s * y; V[k * n + q] = s * x + c * y; }
            }
    }
    int best = 0;
    for (int i = 1; i < n; ++i) if (A[i * n + i] < A[best * n + best]) best = i;
    return best;
}

struct TvCount { int count, sign; };
// the inlier count of model m (in output form) over the pair's list, the same number in every thread (H: under the sign with more inliers, + on a tie)
template <int KIND> __device__ __forceinline__ TvCount tv_count(const float (&m)[9], const f32x4* corr, int S, float t2, int* red8) {
    int pos = 0, neg = 0;
    for (int k = threadIdx.x; k < S; k += TV_THREADS) { const int in = tv_test<KIND>(m, corr[k], t2); pos += in > 0; neg += in < 0; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o, 64); neg += __shfl_xor(neg, o, 64); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red8[threadIdx.x >> 6] = pos; red8[4 + (threadIdx.x >> 6)] = neg; }
    __syncthreads();
    pos = red8[0] + red8[1] + red8[2] + red8[3]; neg = red8[4] + red8[5] + red8[6] + red8[7];
    return pos >= neg ? TvCount{pos, 1} : TvCount{neg, -1};
}

}  // namespace lg
