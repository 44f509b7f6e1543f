// lightglue_amd — camera centres and track points from the viewing rays of every observation, the rotations kept (lg_positioning_solve; the definition is in
// include/lightglue_amd.h).  Launches per call:
//   pos_init      one lane per image and track: the image's record, flags and centre (a held image's -R^T t), its status; the track's counters cleared;
//   pos_count     one lane per node: its outputs cleared, its state (0, 2) or "candidate" with its ray, the candidates of every track counted by integer atomicAdd;
//   pos_scan      ONE workgroup: an exclusive scan over the tracks gives every listed track the offset of its list;
//   pos_fill      one lane per node: states 3 / 4, or a place in the track's list by atomicAdd on its cursor (arrival order is arbitrary);
//   pos_sort      one lane per track: the list put into ascending node order (what the atomics left is gone), the image of every entry;
//   pos_take_part ONE workgroup, one lane per image, tracks and nodes strided: the gauge test, the peeling, the search from the held images;
//   per iteration: pos_points (one lane per track: rho, V, g, Vi), pos_reduce (one workgroup per image: its block row of S and its right-hand side),
//   pos_chol_diag + pos_chol_rows once per panel (bodies in lg_cholesky.h), pos_centres (ONE workgroup: substitution, the step, the record), pos_update
//   (one lane per track: its point);
//   pos_classify  one lane per track: the angles, inliers and outliers, the point or none, the node outputs;
//   pos_output    one lane per image: pose and state; lane 0 the summary.
// That is 8 + n (4 + 2 ceil(3 K / 48)) launches for n iterations over K images.  No kernel waits on another workgroup; every kernel of an iteration returns
// at once when the record says the stage has ended (uniform over the grid: only pos_take_part and pos_centres write it).  No floating-point atomics: every sum
// runs in the fixed order the header names.  The track lists (scan / fill / sort, track_listed) and the ray steps (ray_block, ray_apply, ray_angle, ray_weight)
// are lg_solver_steps.h's, shared with lg_bundle.hip and lg_posegraph.hip.  Small matrices are indexed statically (no scratch: profiles/global_positioning.md).
#include <algorithm>
#include <cmath>
#include <string>

#include "lg_cholesky.h"
#include "lg_host_call.h"
#include "lg_kernels.h"
#include "lg_solve3.h"
#include "lg_solver_steps.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr int POS_THREADS = 256, POS_SCAN_THREADS = 1024, POS_SCAN_WAVES = POS_SCAN_THREADS / 64;
constexpr int POS_TILE = 128, POS_STAGE = 16;                // reduce: rows of image a per LDS tile (half the threads: a group of rows is at least one row), list entries
                                                             // of a row's track kept in LDS next to it (a longer list goes on in global memory)
constexpr double POS_DEG = 180.0 / 3.14159265358979323846, POS_FLOOR = 1e-10;
static_assert(POS_THREADS == CH_THREADS && LG_BA_MAX_IMAGES <= POS_THREADS && LG_BA_CHOLESKY_BLOCK == CH_NB, "one lane per image; the Cholesky's workgroup");
constexpr int POS_OK = 1, POS_HELD = 2, POS_IN = 4, POS_LOST = 8;        // image flags: passes the rules, held, takes part, left as "not connected"
constexpr int TRK_OUT = 0, TRK_IN = 1, TRK_LOST = 2, TRK_DEGENERATE = 3; // track states

// off: the gauge test failed (nothing is solved); last: the iteration the stage ended with (-1: it runs); csel: the buffer that holds the newest centres
struct PosHead { int off, last, iters, fail, pos_bad, csel, degenerate, npoints, noutliers, pad[7]; };
static_assert(sizeof(PosHead) <= 256, "the record of the call is 256 bytes");
struct PosImage { double cam[4], R[9], c[3]; };
static_assert(sizeof(PosImage) == 128, "lg_positioning_workspace_bytes counts 128 bytes");

struct PosArgs {
    int n, images, nodes, tracks, iterations;
    double scale, max_angle;                                // radians, degrees
    const float* kpts; const int* num; const long long* track_id; const float* cameras; const float* poses; const unsigned char* constant;
    PosHead* head; PosImage* rec; int* iflag; double* cen; double* S;                          // cen [2][images][3], S [3 images + 1][3 images]
    int* list; int* limg; double* ray; double* rho;                                             // per list entry: node, image; per node: ray [3], rho
    int* tcnt; int* toff; int* tcur; int* tin; int* treach; double* X; double* Vinv; double* g; // per track
    float* poses_out; float* xyz; float* points3d; long long* track_id_out; unsigned char* node_state; unsigned char* image_state; float* angle_error;
    double* summary; int* status;
};

__device__ __forceinline__ bool pos_stopped(const PosArgs& a, int it) { const PosHead& h = *a.head; return h.off || (h.last >= 0 && it > h.last); }
__device__ __forceinline__ bool pos_free(int flag) { return (flag & POS_IN) && !(flag & POS_HELD); }
__device__ __forceinline__ const double* pos_centre(const PosArgs& a, int which, int k) { return a.cen + ((long long)which * a.images + k) * 3; }

// ------------------------------------------------------------------ records
__global__ __launch_bounds__(POS_THREADS) void pos_init_kernel(PosArgs a) {
    const long long g = (long long)blockIdx.x * POS_THREADS + threadIdx.x;
    if (g == 0) { PosHead h{}; h.last = -1; *a.head = h; }
    if (g < a.images) {
        const int k = (int)g;
        const float* c = a.cameras + (long long)k * 4;
        const float* p = a.poses + (long long)k * 12;
        const bool held = a.constant[k] != 0;
        bool ok = camera_ok(c);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int e = 0; e < 3; ++e) ok = ok && isfinite(p[4 * r + e]);
            if (held) ok = ok && isfinite(p[4 * r + 3]);
        }
        PosImage im{};
#pragma unroll
        for (int e = 0; e < 4; ++e) im.cam[e] = (double)c[e];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int e = 0; e < 3; ++e) im.R[3 * r + e] = ok ? (double)p[4 * r + e] : 0.0;
        if (ok && held) {
            const double t[3] = {(double)p[3], (double)p[7], (double)p[11]};
#pragma unroll
            for (int e = 0; e < 3; ++e) im.c[e] = -((im.R[e] * t[0] + im.R[3 + e] * t[1]) + im.R[6 + e] * t[2]);
        }
        a.rec[k] = im;
        a.iflag[k] = (ok ? POS_OK : 0) | (held ? POS_HELD : 0);
#pragma unroll
        for (int e = 0; e < 3; ++e) { a.cen[(long long)k * 3 + e] = im.c[e]; a.cen[((long long)a.images + k) * 3 + e] = im.c[e]; }
        a.status[k] = ok ? LG_OK : LG_ERR_CAMERA;
    }
    if (g < a.tracks) {
        a.tcnt[g] = 0; a.tcur[g] = 0; a.toff[g] = 0; a.tin[g] = TRK_OUT; a.treach[g] = 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) a.X[g * 3 + e] = 0.0;
    }
}

// ------------------------------------------------------------------ candidates and their rays
__global__ __launch_bounds__(POS_THREADS) void pos_count_kernel(PosArgs a) {
    const int v = blockIdx.x * POS_THREADS + threadIdx.x;
    if (v >= a.nodes) return;
    const int k = v / a.n, i = v - k * a.n;
    const float nanf_ = __builtin_nanf("");
    a.points3d[(long long)v * 3] = nanf_; a.points3d[(long long)v * 3 + 1] = nanf_; a.points3d[(long long)v * 3 + 2] = nanf_;
    a.track_id_out[v] = -1; a.angle_error[v] = nanf_;
    int state = 0;
    const long long j = a.track_id[v];
    if (i < live_rows(a.num, k, a.n) && j >= 0 && j < a.tracks) {
        if (!(a.iflag[k] & POS_OK)) state = 2;
        else {
            const PosImage& im = a.rec[k];
            const double ux = ((double)a.kpts[(long long)v * 2] - im.cam[2]) / im.cam[0], uy = ((double)a.kpts[(long long)v * 2 + 1] - im.cam[3]) / im.cam[1];
            double w[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) w[e] = (im.R[e] * ux + im.R[3 + e] * uy) + im.R[6 + e];
            const double nrm = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);      // of the rotated vector: a float32 R is orthonormal to 1e-7 only
#pragma unroll
            for (int e = 0; e < 3; ++e) a.ray[(long long)v * 3 + e] = w[e] / nrm;
            state = 1;
            atomicAdd(a.tcnt + j, 1);
        }
    }
    a.node_state[v] = (unsigned char)state;
}

// the lists of the listed tracks (lg_solver_steps.h): ONE workgroup scans; one lane per node fills (states 4 / 3); one lane per track sorts
__global__ __launch_bounds__(POS_SCAN_THREADS) void pos_scan_kernel(PosArgs a) {
    __shared__ int sh[POS_SCAN_WAVES];
    track_scan<POS_SCAN_THREADS>(a, sh);
}
__global__ __launch_bounds__(POS_THREADS) void pos_fill_kernel(PosArgs a) { track_fill<4, 3>(a, blockIdx.x * POS_THREADS + threadIdx.x); }
__global__ __launch_bounds__(POS_THREADS) void pos_sort_kernel(PosArgs a) { track_sort(a, blockIdx.x * POS_THREADS + threadIdx.x); }

// ------------------------------------------------------------------ who takes part: ONE workgroup, lane i = image i, tracks and nodes strided
// The gauge: at least two held images that pass the rules, not all at one centre; otherwise nothing is solved.  Peeling: removal is monotone, so the set left
// when nothing changes does not depend on the order of the removals (tracks first, then images, per round here).  Then the search from the held images.
__global__ __launch_bounds__(POS_THREADS) void pos_take_part_kernel(PosArgs a) {
    __shared__ int in[POS_THREADS], reach[POS_THREADS], lo[POS_THREADS], hi[POS_THREADS], first;
    const int i = threadIdx.x, K = a.images;
    const bool mine = i < K;
    const int flag = mine ? a.iflag[i] : 0;
    const bool hok = (flag & POS_OK) && (flag & POS_HELD);
    if (i == 0) first = POS_THREADS;
    __syncthreads();
    if (hok) atomicMin(&first, i);
    const int held = __syncthreads_count(hok);
    bool apart = false;
    if (hok && held >= 2) {
        const double* c = a.rec[i].c;
        const double* f = a.rec[first].c;
        apart = c[0] != f[0] || c[1] != f[1] || c[2] != f[2];
    }
    if (!__syncthreads_or(apart)) {                         // (uniform) no gauge
        if (i == 0) { a.head->off = 1; a.head->pos_bad = 1; }
        return;
    }
    in[i] = (flag & POS_OK) ? 1 : 0;
    for (int j = i; j < a.tracks; j += POS_THREADS) a.tin[j] = track_listed(a, j) ? TRK_IN : TRK_OUT;
    __syncthreads();
    for (;;) {
        int changed = 0;
        for (int j = i; j < a.tracks; j += POS_THREADS) {
            if (a.tin[j] != TRK_IN) continue;
            const int off = a.toff[j], len = a.tcnt[j];
            int last = -1, cnt = 0;
            for (int q = 0; q < len && cnt < 2; ++q) { const int k = a.limg[off + q]; if (k != last && in[k]) { ++cnt; last = k; } }
            if (cnt < 2) { a.tin[j] = TRK_OUT; changed = 1; }
        }
        lo[i] = 0x7FFFFFFF; hi[i] = -1;
        __syncthreads();
        for (int v = i; v < a.nodes; v += POS_THREADS) {     // per image the lowest and the highest label still there: two tracks iff they differ
            if (a.node_state[v] != 1) continue;
            const int j = (int)a.track_id[v];
            if (a.tin[j] != TRK_IN) continue;
            const int k = v / a.n;
            atomicMin(&lo[k], j); atomicMax(&hi[k], j);
        }
        __syncthreads();
        int nxt = in[i];
        if (in[i] && !(flag & POS_HELD) && !(hi[i] > lo[i])) nxt = 0;
        changed = __syncthreads_or(changed || nxt != in[i]);
        in[i] = nxt;
        __syncthreads();
        if (!changed) break;
    }
    reach[i] = in[i] && hok;
    __syncthreads();
    for (;;) {
        int changed = 0;
        for (int j = i; j < a.tracks; j += POS_THREADS) {
            if (a.tin[j] != TRK_IN || a.treach[j]) continue;
            const int off = a.toff[j], len = a.tcnt[j];
            for (int q = 0; q < len; ++q) { const int k = a.limg[off + q]; if (in[k] && reach[k]) { a.treach[j] = 1; changed = 1; break; } }
        }
        hi[i] = 0;
        __syncthreads();
        for (int v = i; v < a.nodes; v += POS_THREADS) {
            if (a.node_state[v] != 1) continue;
            const int j = (int)a.track_id[v];
            if (a.tin[j] == TRK_IN && a.treach[j]) hi[v / a.n] = 1;      // (every writer stores 1)
        }
        __syncthreads();
        const int nxt = reach[i] || (in[i] && hi[i]);
        changed = __syncthreads_or(changed || nxt != reach[i]);
        reach[i] = nxt;
        __syncthreads();
        if (!changed) break;
    }
    for (int j = i; j < a.tracks; j += POS_THREADS) if (a.tin[j] == TRK_IN && !a.treach[j]) a.tin[j] = TRK_LOST;
    if (mine) a.iflag[i] = flag | (in[i] && reach[i] ? POS_IN : 0) | (in[i] && !reach[i] ? POS_LOST : 0);
}

// ------------------------------------------------------------------ per iteration 1: one lane per track: rho of its observations, V, g, Vi
__global__ __launch_bounds__(POS_THREADS) void pos_points_kernel(PosArgs a, int it, double s_it) {
    if (pos_stopped(a, it)) return;
    const int j = blockIdx.x * POS_THREADS + threadIdx.x;
    if (j >= a.tracks || a.tin[j] != TRK_IN) return;
    const int len = a.tcnt[j], off = a.toff[j], cur = it & 1;
    const double X[3] = {a.X[(long long)j * 3], a.X[(long long)j * 3 + 1], a.X[(long long)j * 3 + 2]};
    double V[6] = {0, 0, 0, 0, 0, 0}, G[3] = {0, 0, 0};
    for (int q = 0; q < len; ++q) {
        const int v = a.list[off + q], k = a.limg[off + q], flag = a.iflag[k];
        if (!(flag & POS_IN)) continue;
        const double* ray = a.ray + (long long)v * 3;
        const double* c = pos_centre(a, cur, k);
        double rho = 1.0;
        if (it > 0) {
            const double e[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
            rho = ray_weight(ray, e, s_it);
        }
        a.rho[v] = rho;
        double M[6];
        ray_block(ray, rho, M);
#pragma unroll
        for (int e = 0; e < 6; ++e) V[e] += M[e];
        if (flag & POS_HELD) {
            double y[3];
            ray_apply(M, c, y);
#pragma unroll
            for (int e = 0; e < 3; ++e) G[e] += y[e];
        }
    }
    double Vi[3][3];
    const bool ok = tri_inverse3(V, Vi);
    double* vo = a.Vinv + (long long)j * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vo[3 * r + c] = ok ? Vi[r][c] : 0.0;
        a.g[(long long)j * 3 + r] = G[r];
    }
    if (!ok) { a.tin[j] = TRK_DEGENERATE; atomicAdd(&a.head->degenerate, 1); }      // out for the rest of the call
}

// ------------------------------------------------------------------ per iteration 2: the block row of image ia and its right-hand side
// Thread t = (column image b = t mod Kp, part = t / Kp), Kp the smallest power of two >= images: with few images the rows are shared out, so that all lanes
// work.  POS_TILE rows of image ia at a time go through LDS: the lane of a row stages M_a, Y = M_a Vi and Y g of its observation and the head of its track's list.
// Then thread (b, part), b <= ia, walks ITS group of G = Kp / 2 consecutive staged rows in ascending order and, for each, the track's list in order, and adds
// Y M_b for every entry of image b (the list is sorted by image: it stops behind them); the threads of column ia do the same for U and the right-hand side.
// The groups' sums go through LDS and thread (b, 0) adds them to its total in ascending order.  One thread owns one sum: the order of every sum is fixed
// (the header: groups of G rows).
__global__ __launch_bounds__(POS_THREADS) void pos_reduce_kernel(PosArgs a, int it) {
    __shared__ double sY[POS_TILE][9], sM[POS_TILE][6], sYg[POS_TILE][3], sPart[POS_THREADS][9], sUp[POS_TILE][9];
    __shared__ int sOff[POS_TILE], sLen[POS_TILE], sImg[POS_TILE][POS_STAGE], sNode[POS_TILE][POS_STAGE];
    if (pos_stopped(a, it)) return;
    const int ia = blockIdx.x, t = threadIdx.x, K = a.images, dim = 3 * K;
    int Kp = 2;
    while (Kp < K) Kp <<= 1;                                // <= POS_THREADS
    const int b = t & (Kp - 1), part = t / Kp, parts = POS_THREADS / Kp, group = POS_TILE / parts;      // group = Kp / 2 >= 1; parts <= POS_TILE
    const bool free_a = pos_free(a.iflag[ia]), lower = b <= ia;            // ia < images <= Kp
    const bool free_b = lower && pos_free(a.iflag[b]), own = b == ia;
    double* out = a.S + ((long long)3 * ia * dim + 3 * b);
    double* z = a.S + (long long)dim * dim + 3 * ia;
    if (!free_a) {                                          // the image's columns drop out: identity, zero coupling, zero right-hand side
        if (lower && part == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(long long)r * dim + c] = (own && r == c) ? 1.0 : 0.0;
            if (own) { z[0] = 0.0; z[1] = 0.0; z[2] = 0.0; }
        }
        return;
    }
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, U[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // U: its upper triangle (6), then the right-hand side (3)
    for (int i0 = 0; i0 < a.n; i0 += POS_TILE) {
        __syncthreads();                                    // the previous tile and its groups' sums have been read
        if (t < POS_TILE) {
            const int i = i0 + t;
            const long long v = (long long)ia * a.n + i;
            int len = 0, off = 0;
            if (i < a.n && a.node_state[v] == 1) {
                const int j = (int)a.track_id[v];
                if (a.tin[j] == TRK_IN) {
                    len = a.tcnt[j]; off = a.toff[j];
                    double M[6];
                    ray_block(a.ray + v * 3, a.rho[v], M);
                    const double* Vi = a.Vinv + (long long)j * 9;
                    const double* g = a.g + (long long)j * 3;
                    const double Mf[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
#pragma unroll
                    for (int e = 0; e < 6; ++e) sM[t][e] = M[e];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        double y[3];
#pragma unroll
                        for (int m = 0; m < 3; ++m) { y[m] = (Mf[r][0] * Vi[m] + Mf[r][1] * Vi[3 + m]) + Mf[r][2] * Vi[6 + m]; sY[t][3 * r + m] = y[m]; }
                        sYg[t][r] = (y[0] * g[0] + y[1] * g[1]) + y[2] * g[2];
                    }
                }
            }
            sLen[t] = len; sOff[t] = off;
            for (int l = 0; l < min(len, POS_STAGE); ++l) { sImg[t][l] = a.limg[off + l]; sNode[t][l] = a.list[off + l]; }
        }
        __syncthreads();
        const int q0 = part * group, q1 = min(q0 + group, min(POS_TILE, a.n - i0));
        double p[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (free_b) {
            for (int q = q0; q < q1; ++q) {
                const int len = sLen[q], off = sOff[q];
                for (int l = 0; l < len; ++l) {
                    const int k = l < POS_STAGE ? sImg[q][l] : a.limg[off + l];
                    if (k > b) break;
                    if (k < b) continue;
                    const int v = l < POS_STAGE ? sNode[q][l] : a.list[off + l];
                    double M[6];
                    ray_block(a.ray + (long long)v * 3, a.rho[v], M);
                    const double Mf[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) p[3 * r + c] += (sY[q][3 * r] * Mf[0][c] + sY[q][3 * r + 1] * Mf[1][c]) + sY[q][3 * r + 2] * Mf[2][c];
                }
            }
        }
        if (own) {
            for (int q = q0; q < q1; ++q) {
                if (!sLen[q]) continue;
#pragma unroll
                for (int e = 0; e < 6; ++e) pu[e] += sM[q][e];
#pragma unroll
                for (int e = 0; e < 3; ++e) pu[6 + e] += sYg[q][e];
            }
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) sPart[t][e] = p[e];
        if (own) {
#pragma unroll
            for (int e = 0; e < 9; ++e) sUp[part][e] = pu[e];
        }
        __syncthreads();
        if (part == 0 && free_b) {
            for (int pp = 0; pp < parts; ++pp) {
#pragma unroll
                for (int e = 0; e < 9; ++e) acc[e] += sPart[pp * Kp + b][e];
            }
        }
        if (part == 0 && own) {
            for (int pp = 0; pp < parts; ++pp) {
#pragma unroll
                for (int e = 0; e < 9; ++e) U[e] += sUp[pp][e];
            }
        }
    }
    if (part != 0) return;
    if (lower) {
        const double Uf[3][3] = {{U[0], U[1], U[2]}, {U[1], U[3], U[4]}, {U[2], U[4], U[5]}};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(long long)r * dim + c] = !free_b ? 0.0 : own ? Uf[r][c] - acc[3 * r + c] : -acc[3 * r + c];
    }
    if (own) { z[0] = U[6]; z[1] = U[7]; z[2] = U[8]; }
}

// ------------------------------------------------------------------ per iteration 3: the Cholesky of lg_cholesky.h, pivot floor 1e-10 as in lg_posegraph.hip
__global__ __launch_bounds__(CH_THREADS) void pos_chol_diag_kernel(PosArgs a, int it, int panel) {
    __shared__ CholeskyDiagLds m;
    if (pos_stopped(a, it)) return;
    cholesky_diag(a.S, 3 * a.images, panel, POS_FLOOR, &a.head->fail, m);
}
__global__ __launch_bounds__(CH_THREADS) void pos_chol_rows_kernel(PosArgs a, int it, int panel) {
    __shared__ CholeskyRowsLds m;
    if (pos_stopped(a, it)) return;
    cholesky_rows(a.S, 3 * a.images, 1, panel, panel + blockIdx.x, m);
}

// ------------------------------------------------------------------ per iteration 4: ONE workgroup: the centres, the step, a failed pivot, the end of the stage
__global__ __launch_bounds__(POS_THREADS) void pos_centres_kernel(PosArgs a, int it, int final_scale) {
    __shared__ double sd[3 * LG_BA_MAX_IMAGES], red[POS_THREADS];
    __shared__ CholeskySolveLds m;
    if (pos_stopped(a, it)) return;
    const int i = threadIdx.x, K = a.images, cur = it & 1;
    cholesky_backsolve(a.S, 3 * K, 1, sd, m);
    double mx = 0.0;
    int bad = 0;
    if (i < K) {
        const double* old = pos_centre(a, cur, i);
        double* now = a.cen + ((long long)(cur ^ 1) * K + i) * 3;
        const bool fr = pos_free(a.iflag[i]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double x = fr ? sd[3 * i + r] : old[r], step = fabs(x - old[r]);
            if (!isfinite(step)) bad = 1;
            mx = fmax(mx, step);
            now[r] = x;
        }
    }
    red[i] = mx;
    bad = __syncthreads_or(bad);
    if (i == 0) {
        for (int q = 1; q < POS_THREADS; ++q) mx = fmax(mx, red[q]);
        PosHead& h = *a.head;
        h.iters = it + 1; h.csel = cur ^ 1;
        if (h.fail) h.pos_bad = 1;
        h.fail = 0;
        if (final_scale && !bad && mx < 1e-12) h.last = it;    // this iteration's points are still written; later launches return at once
    }
}

// ------------------------------------------------------------------ per iteration 5: one lane per track: its point from the new centres
__global__ __launch_bounds__(POS_THREADS) void pos_update_kernel(PosArgs a, int it) {
    if (pos_stopped(a, it)) return;
    const int j = blockIdx.x * POS_THREADS + threadIdx.x;
    if (j >= a.tracks || a.tin[j] != TRK_IN) return;
    const int len = a.tcnt[j], off = a.toff[j], now = (it & 1) ^ 1;
    double acc[3] = {a.g[(long long)j * 3], a.g[(long long)j * 3 + 1], a.g[(long long)j * 3 + 2]};
    for (int q = 0; q < len; ++q) {
        const int v = a.list[off + q], k = a.limg[off + q];
        if (!pos_free(a.iflag[k])) continue;
        double M[6], y[3];
        ray_block(a.ray + (long long)v * 3, a.rho[v], M);
        ray_apply(M, pos_centre(a, now, k), y);
#pragma unroll
        for (int e = 0; e < 3; ++e) acc[e] += y[e];
    }
    const double* Vi = a.Vinv + (long long)j * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) a.X[(long long)j * 3 + r] = (Vi[3 * r] * acc[0] + Vi[3 * r + 1] * acc[1]) + Vi[3 * r + 2] * acc[2];
}

// ------------------------------------------------------------------ the final state: one lane per track
__global__ __launch_bounds__(POS_THREADS) void pos_classify_kernel(PosArgs a) {
    const int j = blockIdx.x * POS_THREADS + threadIdx.x;
    if (j >= a.tracks) return;
    const float nanf_ = __builtin_nanf("");
    float* xo = a.xyz + (long long)j * 3;
    xo[0] = nanf_; xo[1] = nanf_; xo[2] = nanf_;
    if (!track_listed(a, j)) return;                          // its nodes carry 3 or 4 already
    const PosHead h = *a.head;
    const int len = a.tcnt[j], off = a.toff[j], tin = a.tin[j];
    if (tin != TRK_IN || h.pos_bad) {
        for (int q = 0; q < len; ++q) {
            const int v = a.list[off + q], in = a.iflag[a.limg[off + q]] & POS_IN;
            a.node_state[v] = (unsigned char)(tin == TRK_OUT ? 4 : tin == TRK_LOST ? 5 : tin == TRK_DEGENERATE ? (in ? 6 : 4) : in ? 9 : 4);
        }
        return;
    }
    const double X[3] = {a.X[(long long)j * 3], a.X[(long long)j * 3 + 1], a.X[(long long)j * 3 + 2]};
    int images = 0, last = -1, outliers = 0;
    for (int q = 0; q < len; ++q) {
        const int v = a.list[off + q], k = a.limg[off + q];
        if (!(a.iflag[k] & POS_IN)) { a.node_state[v] = 4; continue; }
        const double* c = pos_centre(a, h.csel, k);
        const double e[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
        double ve;
        const double phi = ray_angle(a.ray + (long long)v * 3, e, ve) * POS_DEG;
        const bool inlier = ve > 0.0 && phi <= a.max_angle;
        a.angle_error[v] = (float)phi;
        a.node_state[v] = inlier ? 1 : 7;
        if (!inlier) ++outliers;
        else if (k != last) { ++images; last = k; }
    }
    const bool has = images >= 2;
    for (int q = 0; q < len; ++q) {
        const int v = a.list[off + q];
        if (a.node_state[v] != 1) continue;
        if (!has) { a.node_state[v] = 8; continue; }
        a.track_id_out[v] = j;
#pragma unroll
        for (int e = 0; e < 3; ++e) a.points3d[(long long)v * 3 + e] = (float)X[e];
    }
    if (has) {
        xo[0] = (float)X[0]; xo[1] = (float)X[1]; xo[2] = (float)X[2];
        atomicAdd(&a.head->npoints, 1);
    }
    if (outliers) atomicAdd(&a.head->noutliers, outliers);
}

__global__ __launch_bounds__(POS_THREADS) void pos_output_kernel(PosArgs a) {
    const int k = blockIdx.x * POS_THREADS + threadIdx.x;
    const PosHead h = *a.head;
    const float nanf_ = __builtin_nanf("");
    if (k == 0) {
        int posed = 0;
        for (int q = 0; q < a.images; ++q) { const int f = a.iflag[q]; posed += (f & POS_OK) && ((f & POS_HELD) || ((f & POS_IN) && !h.pos_bad)); }
        a.summary[0] = (double)posed; a.summary[1] = (double)h.npoints; a.summary[2] = (double)h.noutliers; a.summary[3] = (double)h.iters;
        a.summary[4] = h.pos_bad ? 0.0 : 1.0; a.summary[5] = h.off ? 0.0 : 1.0; a.summary[6] = (double)h.degenerate; a.summary[7] = 0.0;
    }
    if (k >= a.images) return;
    const int f = a.iflag[k];
    const bool ok = f & POS_OK, held = f & POS_HELD, in = f & POS_IN, posed = ok && !held && in && !h.pos_bad;
    const float* p = a.poses + (long long)k * 12;
    float* o = a.poses_out + (long long)k * 12;
    const double* R = a.rec[k].R;
    const double* c = pos_centre(a, h.csel, k);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int e = 0; e < 3; ++e) o[4 * r + e] = ok ? p[4 * r + e] : nanf_;
        o[4 * r + 3] = !ok ? nanf_ : held ? p[4 * r + 3] : posed ? (float)minus_Rc(R, c, r) : nanf_;
    }
    a.image_state[k] = (unsigned char)(!ok ? 4 : held ? 1 : posed ? 0 : in ? 5 : (f & POS_LOST) ? 3 : 2);
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_positioning_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags) {
    PosLayout L;
    return pos_layout(images, n, tracks, flags, L) ? -1 : L.total;
}

int lg_positioning_solve(const lg_positioning_io* io, void* hip_stream) {
    static const char* const stage = "lg_positioning_solve";
    const auto refuse = [](const char* why) { return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why); };
    if (!io) return refuse("null io");
    PosLayout L;
    if (const char* why = pos_layout(io->images, io->n, io->tracks, io->flags, L)) return refuse(why);
    if (const char* why = pos_settings_error(io->num_iterations, io->angle_scale, io->max_angle_error)) return refuse(why);
    if (!io->cameras || !io->poses || !io->constant_pose || !io->poses_out || !io->image_state || !io->summary || !io->status || (io->tracks && !io->xyz) ||
        (L.nodes && (!io->kpts || !io->track_id || !io->points3d || !io->track_id_out || !io->node_state || !io->angle_error)))
        return refuse("null pointer among kpts, track_id, cameras, poses, constant_pose, poses_out, xyz, points3d, track_id_out, node_state, image_state, "
                      "angle_error, summary, status");
    if (const int rc = check_workspace(stage, "lg_positioning_workspace_bytes", io->workspace, io->workspace_bytes, L.total)) return rc;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Carved ws(io->workspace);
    PosArgs a{};
    a.n = io->n; a.images = io->images; a.nodes = (int)L.nodes; a.tracks = io->tracks; a.iterations = io->num_iterations;
    a.scale = io->angle_scale * (3.14159265358979323846 / 180.0); a.max_angle = io->max_angle_error;
    a.kpts = io->kpts; a.num = io->num; a.track_id = reinterpret_cast<const long long*>(io->track_id); a.cameras = io->cameras; a.poses = io->poses;
    a.constant = io->constant_pose;
    a.head = ws.as<PosHead>(L.head); a.rec = ws.as<PosImage>(L.rec); a.iflag = ws.ints(L.iflag); a.cen = ws.f64(L.cen); a.S = ws.f64(L.S);
    a.list = ws.ints(L.list); a.limg = ws.ints(L.limg); a.ray = ws.f64(L.ray); a.rho = ws.f64(L.rho);
    a.tcnt = ws.ints(L.tcnt); a.toff = ws.ints(L.toff); a.tcur = ws.ints(L.tcur); a.tin = ws.ints(L.tin); a.treach = ws.ints(L.treach);
    a.X = ws.f64(L.X); a.Vinv = ws.f64(L.Vinv); a.g = ws.f64(L.g);
    a.poses_out = io->poses_out; a.xyz = io->xyz; a.points3d = io->points3d; a.track_id_out = reinterpret_cast<long long*>(io->track_id_out);
    a.node_state = io->node_state; a.image_state = io->image_state; a.angle_error = io->angle_error; a.summary = io->summary; a.status = io->status;

    auto blocks = [](long long items) { return dim3((unsigned)((items + POS_THREADS - 1) / POS_THREADS)); };
    const dim3 th(POS_THREADS);
    const int K = io->images, T = io->tracks, n = io->num_iterations;
    hipLaunchKernelGGL(pos_init_kernel, blocks(std::max<long long>(K, T)), th, 0, s, a);
    if (L.nodes) hipLaunchKernelGGL(pos_count_kernel, blocks(L.nodes), th, 0, s, a);
    if (T) hipLaunchKernelGGL(pos_scan_kernel, dim3(1), dim3(POS_SCAN_THREADS), 0, s, a);
    if (L.nodes) hipLaunchKernelGGL(pos_fill_kernel, blocks(L.nodes), th, 0, s, a);
    if (T) hipLaunchKernelGGL(pos_sort_kernel, blocks(T), th, 0, s, a);
    hipLaunchKernelGGL(pos_take_part_kernel, dim3(1), th, 0, s, a);
    for (int it = 0; it < n; ++it) {
        const int halvings = std::max(0, n - 6 - it);
        if (T) hipLaunchKernelGGL(pos_points_kernel, blocks(T), th, 0, s, a, it, a.scale * std::ldexp(1.0, halvings));
        hipLaunchKernelGGL(pos_reduce_kernel, dim3(K), th, 0, s, a, it);
        for_cholesky_panels(3 * K, 1, [&](int p, int tiles_below) {
            hipLaunchKernelGGL(pos_chol_diag_kernel, dim3(1), th, 0, s, a, it, p);
            hipLaunchKernelGGL(pos_chol_rows_kernel, dim3(tiles_below), th, 0, s, a, it, p);
        });
        hipLaunchKernelGGL(pos_centres_kernel, dim3(1), th, 0, s, a, it, halvings == 0 ? 1 : 0);
        if (T) hipLaunchKernelGGL(pos_update_kernel, blocks(T), th, 0, s, a, it);
    }
    if (T) hipLaunchKernelGGL(pos_classify_kernel, blocks(T), th, 0, s, a);
    hipLaunchKernelGGL(pos_output_kernel, blocks(K), th, 0, s, a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

}  // extern "C"
