// lightglue_amd — the device code the three hypothesise-and-verify estimators share (lg_twoview.hip, lg_relpose.hip, lg_abspose.hip), every step written once:
//   lists      the compaction of matches0 into a pair's correspondence list (tv_compact_pair) and the Hartley normalisation over a point map (hartley);
//   sampling   the counter-based hash and the M distinct picks (tv_sample);
//   solving    bearing(s), horner<N> (under the 5-point solver's degree-10 and P3P's degree-4 root finders, which stay two: see either file), det3 and ata3;
//   models     the 9-float helpers (output form, unit norm, denormalisation), the division-free F / H inlier test, the broadcast-tile scoring loop;
//   winners    WinnerKey<K, B> (count, ~hypothesis, ~root: 32 bits for the verifier, 64 for the pose estimators) and its wave maximum + atomicMax (publish_winner);
//   refits     accumulate_upper<N> (one row) / accumulate_upper2<N> (two rows: another association, so another function), reduce_upper<N>, the single-lane fp64
//              Jacobi, the null vector of the F / H normal matrix (tv_null_vector), the recount that keeps a refit if it is not worse (tv_keep_if_not_worse);
//   results    the workgroup inlier count (tv_count), the mask of a pair (tv_mark_inliers) and its rows of inliers0 / the verified matches (tv_write_rows).
// The camera rule (camera_ok) is lg_common.h's: the bundle adjuster and the triangulator apply it too.  Everything here is compiled without floating-point
// contraction (the pragma below governs the rest of the including translation unit) and the inlier test is written in explicit fmaf: a model and a decision are
// the same bits in every kernel of the three files, and a shared step keeps the order of operations its copies had.
#pragma once

#include "lg_kernels.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr int TV_THREADS = 256, TV_TILE = LG_TWOVIEW_TILE;
constexpr int TV_H = 0, TV_F = 1;                        // model kinds
static_assert(TV_TILE == TV_THREADS, "a tile is loaded by one float4 per thread");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Hartley { float cx0, cy0, s0, cx1, cy1, s1; };                                 // x -> (x - c) s of either side
struct TvHeader { int count; unsigned key; Hartley n; };                              // 32 bytes per pair
static_assert(sizeof(TvHeader) == 32, "lg_twoview_workspace_bytes counts 32 bytes");

// what the compaction of one pair reads
struct TvSource {
    int n0, n1;
    PairIndex px;                                        // the images pair p reads (lg_common.h)
    const float* kpts0; const float* kpts1; const int* num0; const int* num1;
    const long long* matches0;
};

// ------------------------------------------------------------------ Hartley normalisation of either side of a list under a point map (identity: pixels; bearings):
// centroid and mean distance in fp64 (per-thread strided partial sums, then block_sum), scale sqrt(2) / mean.  Every thread calls; red4: __shared__ double[4]
template <class Map> __device__ __forceinline__ Hartley hartley(const f32x4* corr, int S, Map map, double* red4) {
    const int tid = threadIdx.x;
    double sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;
    for (int k = tid; k < S; k += TV_THREADS) { const f32x4 c = map(corr[k]); sx0 += c[0]; sy0 += c[1]; sx1 += c[2]; sy1 += c[3]; }
    const double inv = S ? 1.0 / S : 0.0;
    const double cx0 = block_sum(sx0, red4) * inv, cy0 = block_sum(sy0, red4) * inv;
    const double cx1 = block_sum(sx1, red4) * inv, cy1 = block_sum(sy1, red4) * inv;
    double d0 = 0, d1 = 0;
    for (int k = tid; k < S; k += TV_THREADS) {
        const f32x4 c = map(corr[k]);
        const double ax = c[0] - cx0, ay = c[1] - cy0, bx = c[2] - cx1, by = c[3] - cy1;
        d0 += sqrt(ax * ax + ay * ay); d1 += sqrt(bx * bx + by * by);
    }
    const double m0 = block_sum(d0, red4) * inv, m1 = block_sum(d1, red4) * inv;
    return {(float)cx0, (float)cy0, m0 > 0 ? (float)(1.4142135623730951 / m0) : 1.f, (float)cx1, (float)cy1, m1 > 0 ? (float)(1.4142135623730951 / m1) : 1.f};
}

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
    TvHeader h;
    h.count = S; h.key = 0u;
    h.n = hartley(corr, S, [](const f32x4& c) { return c; }, red4);
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

// ------------------------------------------------------------------ solving
__device__ __forceinline__ float bearing(float x, float c, float f) { return (x - c) / f; }
// (x0, y0, x1, y1) in pixels -> the bearings under the pinhole cameras (fx, fy, cx, cy) of either side
__device__ __forceinline__ f32x4 bearings(const f32x4& c, const float* cam0, const float* cam1) {
    return f32x4{bearing(c[0], cam0[2], cam0[0]), bearing(c[1], cam0[3], cam0[1]), bearing(c[2], cam1[2], cam1[0]), bearing(c[3], cam1[3], cam1[1])};
}
template <class T> __device__ __forceinline__ T det3(const T* r0, const T* r1, const T* r2) {
    return (r0[0] * (r1[1] * r2[2] - r1[2] * r2[1]) - r0[1] * (r1[0] * r2[2] - r1[2] * r2[0])) + r0[2] * (r1[0] * r2[1] - r1[1] * r2[0]);
}
// J = A^T A of the row-major 3 x 3 matrix A
__device__ __forceinline__ void ata3(const double* A, double* J) {
    for (int p = 0; p < 3; ++p) for (int q = 0; q < 3; ++q) J[p * 3 + q] = (A[p] * A[q] + A[3 + p] * A[3 + q]) + A[6 + p] * A[6 + q];
}
template <int N> __device__ __forceinline__ double horner(const double (&c)[N + 1], double z) {
    double v = c[N];
#pragma unroll
    for (int i = N - 1; i >= 0; --i) v = v * z + c[i];
    return v;
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
template <int KIND, class T> __device__ __forceinline__ void tv_denormalise(T (&m)[9], const Hartley& n) {
    const T cx1 = n.cx1, cy1 = n.cy1, s1 = n.s1;
    tv_right_t0<T>(m, n.s0, n.cx0, n.cy0);
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

// ------------------------------------------------------------------ winners: (count, ~hypothesis, ~root) in one unsigned K with B bits of root, 0 for no inlier, so that
// the maximum is the most inliers, then the lowest hypothesis, then the lowest root.  The verifier's is WinnerKey<unsigned, 2>, the pose estimators' WinnerKey<u64, 4>
template <class K, int B> struct WinnerKey {
    static constexpr unsigned ROOTS = (1u << B) - 1u;
    static __device__ __forceinline__ K make(int count, int hyp, int root) {
        return count > 0 ? ((K)count << (16 + B)) | ((K)(0xFFFFu - (unsigned)hyp) << B) | (K)(ROOTS - (unsigned)root) : (K)0;
    }
    static __device__ __forceinline__ int hyp_of(K key) { return 0xFFFF - (int)((key >> B) & (K)0xFFFFu); }
    static __device__ __forceinline__ int root_of(K key) { return (int)ROOTS - (int)(key & (K)ROOTS); }
};
typedef WinnerKey<unsigned, 2> TvKey;
typedef WinnerKey<unsigned long long, 4> PoseKey;
__device__ __forceinline__ unsigned wave_max(unsigned key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
    return key;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long key) {     // two 32-bit shuffles per step
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(key >> 32), o, 64), lo = (unsigned)__shfl_xor((int)(key & 0xFFFFFFFFull), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other > key ? other : key;
    }
    return key;
}
// the best key of the wave against the pair's: one atomicMax per wave that has a key at all.  Every thread of the wave calls
template <class K> __device__ __forceinline__ void publish_winner(K key, K* best) {
    key = wave_max(key);
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// ------------------------------------------------------------------ finalise: one workgroup per pair
// acc += the upper triangle of r r^T (row by row, N (N + 1) / 2 entries), fp64, one thread's share
template <int N> __device__ __forceinline__ void accumulate_upper(double (&acc)[N * (N + 1) / 2], const double (&r)[N]) {
    int e = 0;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
        for (int q = p; q < N; ++q) { acc[e] += r[p] * r[q]; ++e; }
}
// acc += the upper triangle of r1 r1^T + r2 r2^T, the two products summed first
template <int N> __device__ __forceinline__ void accumulate_upper2(double (&acc)[N * (N + 1) / 2], const double (&r1)[N], const double (&r2)[N]) {
    int e = 0;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
        for (int q = p; q < N; ++q) { acc[e] += r1[p] * r1[q] + r2[p] * r2[q]; ++e; }
}
// the workgroup's sum of every entry, in the entries' order (block_sum), mirrored into the symmetric matrix M (__shared__, `stride` doubles per row) by thread 0
template <int N> __device__ __forceinline__ void reduce_upper(const double (&acc)[N * (N + 1) / 2], double* M, int stride, double* red4) {
    int e = 0;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
        for (int q = p; q < N; ++q) {
            const double s = block_sum(acc[e], red4);
            if (threadIdx.x == 0) { M[p * stride + q] = s; M[q * stride + p] = s; }
            ++e;
        }
}
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

// The least-squares refit up to its null vector: the normal matrix of the inliers of `fin` (those with the sign `sign`) in the coordinates map(c) normalised by
// n — H: two rows per correspondence, F: one —, upper triangle in fp64, summed in a fixed order into JA, and its smallest eigenvector by Jacobi: f, still in
// normalised coordinates, valid in thread 0 alone.  Every thread calls; JA, JV: __shared__ double[81]
template <int KIND, class Map> __device__ __forceinline__ void tv_null_vector(const float (&fin)[9], int sign, const f32x4* corr, int S, float t2, const Hartley& n, Map map,
                                                                             double* JA, double* JV, double* red4, double (&f)[9]) {
    double acc[45];
#pragma unroll
    for (int e = 0; e < 45; ++e) acc[e] = 0.0;
    for (int k = threadIdx.x; k < S; k += TV_THREADS) {
        const f32x4 c = corr[k];
        if (tv_test<KIND>(fin, c, t2) != sign) continue;
        const f32x4 b = map(c);
        const double x = ((double)b[0] - n.cx0) * n.s0, y = ((double)b[1] - n.cy0) * n.s0, u = ((double)b[2] - n.cx1) * n.s1, v = ((double)b[3] - n.cy1) * n.s1;
        if (KIND == TV_H) {
            const double r1[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u}, r2[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
            accumulate_upper2<9>(acc, r1, r2);
        } else {
            const double r1[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
            accumulate_upper<9>(acc, r1);
        }
    }
    reduce_upper<9>(acc, JA, 9, red4);
    if (threadIdx.x == 0) {
        const int col = tv_jacobi(JA, JV, 9);
        for (int e = 0; e < 9; ++e) f[e] = JV[e * 9 + col];
    }
}
// the refit `ref` (__shared__, 9 floats, output form) counted again and kept — cur and fin replaced — if its inlier count does not drop.  Every thread calls
template <int KIND> __device__ __forceinline__ void tv_keep_if_not_worse(const float* ref_sh, const f32x4* corr, int S, float t2, int* red8, TvCount& cur, float (&fin)[9]) {
    float ref[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) ref[e] = ref_sh[e];
    const TvCount again = tv_count<KIND>(ref, corr, S, t2, red8);
    if (again.count >= cur.count) {
        cur = again;
#pragma unroll
        for (int e = 0; e < 9; ++e) fin[e] = ref[e];
    }
}
// mask[] (__shared__, cleared, and a barrier passed since) set at the image-0 row of every inlier of `fin` unless `empty`.  Every thread calls
template <int KIND> __device__ __forceinline__ void tv_mark_inliers(bool empty, const float (&fin)[9], int sign, const f32x4* corr, const int* rows, int S, float t2, unsigned char* mask) {
    if (!empty)
        for (int k = threadIdx.x; k < S; k += TV_THREADS) if (tv_test<KIND>(fin, corr[k], t2) == sign) mask[rows[k]] = 1;
}
// the finished mask (a barrier passed since it was set) as the pair's rows of inliers0 and, where asked for, of the verified matches: matches0 at the inliers, -1 elsewhere
__device__ __forceinline__ void tv_write_rows(int n0, const unsigned char* mask, const long long* matches0, unsigned char* inliers0, long long* matches0_out) {
    for (int i = threadIdx.x; i < n0; i += TV_THREADS) {
        const unsigned char in = mask[i];
        inliers0[i] = in;
        if (matches0_out) matches0_out[i] = in ? matches0[i] : -1;
    }
}

}  // namespace lg
