// lightglue_amd — THE steps the track and pose-graph solvers share (lg_bundle.hip, lg_positioning.hip, lg_posegraph.hip), each written once: the track lists
// (listed / scan / fill / sort), exp of a rotation vector, the ray block rho (I - v v^T) with its product, angle and reweighting, and the image dot of the
// two iterative solvers (image_sum).  Device bodies in the
// pattern of lg_cholesky.h: the callers' kernels are thin wrappers that keep their names, launch shapes and argument blocks.  The track steps are templates on
// the argument block A, which names tracks, nodes, n, track_id, node_state, list, limg, tcnt, toff, tcur (BaArgs and PosArgs do).  Static indices only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)      // the definitions have no fused multiply-add; the including files say the same for what follows

namespace lg {

// ------------------------------------------------------------------ track lists: count (the caller's) / scan / fill / sort
// a track that gets a list: 2 .. LG_BA_MAX_TRACK_LENGTH candidates
template <class A> __device__ __forceinline__ bool track_listed(const A& a, int j) { const int c = a.tcnt[j]; return c >= 2 && c <= LG_BA_MAX_TRACK_LENGTH; }

// ONE workgroup of THREADS: the exclusive scan of the listed tracks' counts gives every listed track the offset of its list; thread t owns the
// ceil(tracks / THREADS) consecutive tracks from t times that (integers: the order of the additions changes nothing)
template <int THREADS, class A> __device__ __forceinline__ void track_scan(const A& a, int (&sh)[THREADS / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int share = (a.tracks + THREADS - 1) / THREADS;
    const int beg = min((int)threadIdx.x * share, a.tracks), end = min(beg + share, a.tracks);
    int mine = 0;
    for (int j = beg; j < end; ++j) if (track_listed(a, j)) mine += a.tcnt[j];
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += sh[w];
    int at = base + inc - mine;                            // the sum of all counts is at most nodes: every node is counted once
    for (int j = beg; j < end; ++j) if (track_listed(a, j)) { a.toff[j] = at; at += a.tcnt[j]; }
}

// node v (one lane each): a candidate (state 1) of a track without a list takes state SHORT or LONG; any other takes a place in its track's list by
// atomicAdd on the cursor (arrival order is arbitrary) and the answer is true
template <int SHORT, int LONG, class A> __device__ __forceinline__ bool track_fill(const A& a, int v) {
    if (v >= a.nodes) return false;
    if (a.node_state[v] != 1) return false;
    const int j = (int)a.track_id[v], cnt = a.tcnt[j];     // a candidate: 0 <= j < tracks
    if (cnt < 2) { a.node_state[v] = SHORT; return false; }
    if (cnt > LG_BA_MAX_TRACK_LENGTH) { a.node_state[v] = LONG; return false; }
    const int at = atomicAdd(a.tcur + j, 1);
    if (at < cnt) a.list[a.toff[j] + at] = v;              // always: cnt candidates carry this track; toff + cnt <= nodes
    return true;
}

// track j (one lane each): its list put into ascending node order (what the atomics left is gone), the image of every entry
template <class A> __device__ __forceinline__ void track_sort(const A& a, int j) {
    if (j >= a.tracks || !track_listed(a, j)) return;
    const int len = a.tcnt[j];
    int* lst = a.list + a.toff[j];
    for (int q = 1; q < len; ++q) {                        // insertion sort; len <= 1024
        const int key = lst[q];
        int r = q - 1;
        while (r >= 0 && lst[r] > key) { lst[r + 1] = lst[r]; --r; }
        lst[r + 1] = key;
    }
    int* img = a.limg + a.toff[j];
    for (int q = 0; q < len; ++q) img[q] = lst[q] / a.n;
}

// ------------------------------------------------------------------ rotations
// Q = exp([w]x) = I + sin(th) [k]x + (1 - cos(th)) [k]x^2, th = |w|, k = w / th (Rodrigues); the identity at w = 0.  3 x 3 row-major
__device__ __forceinline__ void so3_exp(const double* w, double (&Q)[9]) {
    const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int e = 0; e < 9; ++e) Q[e] = (e % 4 == 0) ? 1.0 : 0.0;
    if (th > 0.0) {
        const double kx = w[0] / th, ky = w[1] / th, kz = w[2] / th, sn = sin(th), c1 = 1.0 - cos(th);
        const double Kx[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double kk = (Kx[3 * i] * Kx[j] + Kx[3 * i + 1] * Kx[3 + j]) + Kx[3 * i + 2] * Kx[6 + j];
                Q[3 * i + j] = (Q[3 * i + j] + sn * Kx[3 * i + j]) + c1 * kk;
            }
    }
}
// row r of t = -R c
__device__ __forceinline__ double minus_Rc(const double* R, const double* c, int r) { return -((R[3 * r] * c[0] + R[3 * r + 1] * c[1]) + R[3 * r + 2] * c[2]); }

// ------------------------------------------------------------------ a ray v (a unit vector) against the vector e from its camera's centre to its point
// M = rho (I - v v^T) as its upper triangle (xx, xy, xz, yy, yz, zz)
__device__ __forceinline__ void ray_block(const double* v, double rho, double (&M)[6]) {
    M[0] = rho * (1.0 - v[0] * v[0]); M[1] = rho * (0.0 - v[0] * v[1]); M[2] = rho * (0.0 - v[0] * v[2]);
    M[3] = rho * (1.0 - v[1] * v[1]); M[4] = rho * (0.0 - v[1] * v[2]); M[5] = rho * (1.0 - v[2] * v[2]);
}
// M x, each row (m0 x0 + m1 x1) + m2 x2
__device__ __forceinline__ void ray_apply(const double (&M)[6], const double* x, double (&y)[3]) {
    y[0] = (M[0] * x[0] + M[1] * x[1]) + M[2] * x[2];
    y[1] = (M[1] * x[0] + M[3] * x[1]) + M[4] * x[2];
    y[2] = (M[2] * x[0] + M[4] * x[1]) + M[5] * x[2];
}
// v . e and phi = atan2(|e - (v . e) v|, v . e)
__device__ __forceinline__ double ray_angle(const double* v, const double (&e)[3], double& ve) {
    ve = (v[0] * e[0] + v[1] * e[1]) + v[2] * e[2];
    const double r[3] = {e[0] - ve * v[0], e[1] - ve * v[1], e[2] - ve * v[2]};
    return atan2(sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]), ve);
}
__device__ __forceinline__ double ray_angle(const double* v, const double (&e)[3]) { double ve; return ray_angle(v, e, ve); }
// the reweighting at scale s: 1 / max(e . e, 1e-12) / (1 + (phi / s)^2)
__device__ __forceinline__ double ray_weight(const double* v, const double (&e)[3], double s) {
    const double ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], q = ray_angle(v, e) / s;
    return 1.0 / fmax(ee, 1e-12) / (1.0 + q * q);
}

// ------------------------------------------------------------------ the image dot of the iterative solvers (lg_bundle_adjust_pcg, lg_posegraph_solve_pcg)
// the images' partials d [images] added in THE fixed order: partial m < 256 = d[m] + d[m + 256] + .. ascending from 0, then a halving tree over the partials.
// Every thread of the (single) workgroup calls it, part holds IMAGE_SUM_PARTIALS doubles; d may have been written by this workgroup before the call
constexpr int IMAGE_SUM_PARTIALS = 256;
__device__ __forceinline__ double image_sum(const double* d, int images, double* part) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < IMAGE_SUM_PARTIALS) {
        double s = 0.0;
        for (int k = t; k < images; k += IMAGE_SUM_PARTIALS) s += d[k];
        part[t] = s;
    }
    __syncthreads();
    for (int h = IMAGE_SUM_PARTIALS / 2; h >= 1; h >>= 1) {
        if (t < h) part[t] += part[t + h];
        __syncthreads();
    }
    return part[0];
}

}  // namespace lg
