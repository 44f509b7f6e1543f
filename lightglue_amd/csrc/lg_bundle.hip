// lightglue_amd — bundle adjustment of poses and points (lg_bundle_adjust; the definition is in include/lightglue_amd.h).  Launches per call:
//   ba_init       one lane per image and track: the image's record, its pose widened, its status; the track's counters cleared, its point widened;
//   ba_count      one lane per node: its state (0, 2, 3, 4) or "candidate", the candidates of every track counted by integer atomicAdd;
//   ba_scan       ONE workgroup: an exclusive scan over the tracks gives every adjusted track the offset of its list;
//   ba_fill       one lane per node: states 5 / 6, or a place in the track's list by atomicAdd on its cursor (arrival order is arbitrary), the image's count;
//   ba_sort       one lane per track: the list put into ascending node order (what the atomics left is gone), the image of every entry;
//   ba_cost + ba_decide   the cost of the input;
//   per iteration: ba_points, ba_reduce, ba_cholesky_diag + ba_cholesky_rows once per panel (bodies in lg_cholesky.h), ba_backsolve, ba_trial_points, ba_cost,
//   ba_decide;
//   ba_scatter    one lane per node, track and image: the outputs.
// lg_bundle_adjust_robust runs the same list per stage with the loss compiled in (ba_linearise<LOSS> is the one weighted linearisation: points, reduce, trial
// points; ba_rho<LOSS> in the cost; the squared instantiation is lg_bundle_adjust's code) and between two stages ba_filter, ba_count<true>, ba_scan, ba_fill,
// ba_sort, ba_cost and ba_restage.  Registers and scratch of every instantiation: profiles/bundle_adjust_robust.md.
// lg_bundle_adjust_focal runs that list with FOCAL compiled in: seven unknowns per image (column 6: the log of a common scale of fx and fy), interleaved per
// image in S; the camera state lives twice like the poses (ba_cam<FOCAL> names the buffer; without FOCAL it is the image's record, which never moves);
// ba_jacobians / ba_linearise fill a seventh column when they are given arrays of 7; the reduce runs 4 column blocks of 49 entries and 28 + 7 + 7 extras and
// overwrites held columns (identity, zero coupling, zero right-hand side); ba_backsolve<true> also writes the trial cameras.  The FOCAL kernels take
// BaFocalArgs, so the other two entry points' kernels keep their argument block (profiles/bundle_adjust_focal.md lists registers and scratch of the FOCAL
// instantiations; profiles/ab_track_solver_steps.md those of the one back substitution).
// lg_bundle_adjust_pcg runs lg_bundle_adjust_robust's list with the solve swapped: ba_pcg_setup (one workgroup per image: U', b, M = S_aa^-1, the start of the
// solve) and, max_cg_iterations times, ba_pcg_tracks (one lane per track: u), ba_pcg_images (one workgroup per image: q = S p, its p.q) and ba_pcg_step (ONE
// workgroup: the dots, alpha, beta, x, r, z, p, the solver's record, the trial poses when the solve ends); S is never formed and its workspace has none
// (profiles/bundle_adjust_pcg.md lists registers and scratch).
// The track lists (scan / fill / sort, "adjusted" = track_listed) and exp of a rotation vector are lg_solver_steps.h's, shared with lg_positioning.hip.
// No kernel waits on another workgroup.  The state lives twice (pose and point buffers 0 / 1): head->sel names the accepted one, a trial is written into the
// other and accepting it flips sel.  Every kernel of an iteration returns at once when head->converged is set (uniform over the grid: only ba_decide writes it).
// No floating-point atomics: every sum runs in the fixed order the header names.  Small matrices are indexed statically (no scratch: profiles/bundle_adjust.md).
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

#include "lg_cholesky.h"
#include "lg_host_call.h"
#include "lg_kernels.h"
#include "lg_solve3.h"
#include "lg_solver_steps.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

// ------------------------------------------------------------------ the sizes, the device records, the kernels' argument blocks, the accessors of the state
constexpr int BA_THREADS = 256, BA_SCAN_THREADS = 1024, BA_SCAN_WAVES = BA_SCAN_THREADS / 64;
constexpr int BA_NB = LG_BA_CHOLESKY_BLOCK;                  // Cholesky (lg_cholesky.h): columns per panel = rows per tile
static_assert(BA_NB == CH_NB && BA_THREADS == CH_THREADS, "lg_cholesky.h is written for 48-column panels and 256 threads");
constexpr int BA_TILE = 32, BA_BCHUNK = 6;                   // reduce: rows of image a per LDS tile, column blocks b per workgroup (6 x 36 = 216 threads)
constexpr int BA_FOCAL_BCHUNK = 4;                           // lg_bundle_adjust_focal: 7 columns per image, 4 x 49 = 196 entry threads and 28 + 7 + 7 extras
template <bool FOCAL> constexpr int BA_COLS = FOCAL ? 7 : 6;
template <bool FOCAL> constexpr int BA_CHUNK = FOCAL ? BA_FOCAL_BCHUNK : BA_BCHUNK;

struct BaHead { double cost, cost_new, lambda, initial_cost; int sel, converged, iters, accepted, fail, nobs, removed, filtered, fstages, pad; };   // removed: by the running filter
static_assert(sizeof(BaHead) <= 256, "the record of the call is 256 bytes");
struct BaImage { double cam[4]; int ok, constant, nact, moved, cconstant, cmoved; double pad2; };   // moved: free in an earlier stage (lg_bundle_adjust_robust);
                                                                                            // cconstant, cmoved: the same of the camera (lg_bundle_adjust_focal)
static_assert(sizeof(BaImage) == 64, "lg_bundle_workspace_bytes counts 64 bytes");

struct BaArgs {
    int n, images, nodes, tracks, dim;
    double lambda0, ftol;
    const float* kpts; const int* num; const long long* track_id; const float* xyz; const float* cameras; const float* poses; const unsigned char* constant;
    BaHead* head; BaImage* rec; double* pose; double* delta; double* icost; double* S;         // pose [2][images][12], S [dim + 1][dim]
    int* list; int* limg; int* tcnt; int* toff; int* tcur; double* X; double* Vinv; double* y;  // X [2][tracks][3]
    float* poses_out; float* xyz_out; float* points3d; unsigned char* node_state; float* obs_err; double* summary; int* status;
    // lg_bundle_adjust_robust, behind everything lg_bundle_adjust's kernels read (their argument offsets stay what they were): the loss scale c, c c, the
    // filter's bar e e, and per track "it moved in an earlier stage" (null without a filter)
    double lc, lc2, fe2; int* tmov;
};
// lg_bundle_adjust_focal: the held cameras (null: none), the camera state (fx, fy, cx, cy) [2][images][4] (head->sel names the accepted one, like the poses),
// cameras_out.  With it delta is [images][7] and S [7 images + 1][7 images].  A type of its own, so that the kernels of the other two entry points keep
// their argument block to the byte (profiles/bundle_adjust_focal.md compares their instruction streams)
struct BaFocalArgs : BaArgs { const unsigned char* cconstant; double* cam; float* cameras_out; };
template <bool FOCAL> using BaArgsOf = std::conditional_t<FOCAL, BaFocalArgs, BaArgs>;

__device__ __forceinline__ bool ba_free(const BaArgs& a, int k) { const BaImage& im = a.rec[k]; return im.ok && !im.constant && im.nact > 0; }
__device__ __forceinline__ bool ba_cam_free(const BaArgs& a, int k) { const BaImage& im = a.rec[k]; return im.ok && !im.cconstant && im.nact > 0; }
// an image with at least one free column
template <bool FOCAL> __device__ __forceinline__ bool ba_any_free(const BaArgs& a, int k) {
    if constexpr (FOCAL) return ba_free(a, k) || ba_cam_free(a, k);
    else return ba_free(a, k);
}
// the camera of image k: with FOCAL buffer `which` of the state, else the record's (it never moves)
template <bool FOCAL> __device__ __forceinline__ const double* ba_cam(const BaArgsOf<FOCAL>& a, int which, int k) {
    if constexpr (FOCAL) return a.cam + ((long long)which * a.images + k) * 4;
    else return a.rec[k].cam;
}
__device__ __forceinline__ const double* ba_pose(const BaArgs& a, int which, int k) { return a.pose + ((long long)which * a.images + k) * 12; }
__device__ __forceinline__ const double* ba_point(const BaArgs& a, int which, int j) { return a.X + ((long long)which * a.tracks + j) * 3; }

// p = R X + t of pose P [12] (R | t row-major 3 x 4)
__device__ __forceinline__ void ba_project(const double* P, const double* X, double (&p)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = ((P[4 * r] * X[0] + P[4 * r + 1] * X[1]) + P[4 * r + 2] * X[2]) + P[4 * r + 3];
}
// the two rows of the pose Jacobian A (2 x 6) and of the point Jacobian B (2 x 3) at p; NA = 7 (lg_bundle_adjust_focal): column 6 is the log focal scale's
template <int NA>
__device__ __forceinline__ void ba_jacobians(const double* P, const double* cam, const double (&p)[3], double (&A0)[NA], double (&A1)[NA], double (&B0)[3], double (&B1)[3]) {
    static_assert(NA == 6 || NA == 7, "six pose columns, or those and the focal column");
    const double iz = 1.0 / p[2], fx = cam[0], fy = cam[1];
    const double ax = fx * iz, az = -(((fx * p[0]) * iz) * iz), by = fy * iz, bz = -(((fy * p[1]) * iz) * iz);
    A0[0] = az * p[1]; A0[1] = ax * p[2] - az * p[0]; A0[2] = -(ax * p[1]); A0[3] = ax; A0[4] = 0.0; A0[5] = az;
    A1[0] = bz * p[1] - by * p[2]; A1[1] = -(bz * p[0]); A1[2] = by * p[0]; A1[3] = 0.0; A1[4] = by; A1[5] = bz;
    if constexpr (NA == 7) { A0[6] = ax * p[0]; A1[6] = by * p[1]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) { B0[e] = ax * P[e] + az * P[8 + e]; B1[e] = by * P[4 + e] + bz * P[8 + e]; }
}
__device__ __forceinline__ void ba_residual(const double* cam, const double (&p)[3], const float* kp, double& rx, double& ry) {
    const double iz = 1.0 / p[2];
    rx = ((cam[0] * p[0]) * iz + cam[2]) - (double)kp[0]; ry = ((cam[1] * p[1]) * iz + cam[3]) - (double)kp[1];
}
__device__ __forceinline__ double ba_damped(double d, double lambda) { return d + lambda * fmin(fmax(d, 1e-6), 1e32); }

// ------------------------------------------------------------------ the loss (lg_bundle_adjust_robust): rho and the weight w of s = rx rx + ry ry
template <int LOSS> __device__ __forceinline__ double ba_rho(const BaArgs& a, double s) {
    if constexpr (LOSS == LG_BA_LOSS_HUBER) return s <= a.lc2 ? s : (2.0 * a.lc) * sqrt(s) - a.lc2;
    else if constexpr (LOSS == LG_BA_LOSS_CAUCHY) return a.lc2 * log1p(s / a.lc2);
    else return s;
}
template <int LOSS> __device__ __forceinline__ double ba_weight(const BaArgs& a, double s) {
    if constexpr (LOSS == LG_BA_LOSS_HUBER) return s <= a.lc2 ? 1.0 : a.lc / sqrt(s);
    else if constexpr (LOSS == LG_BA_LOSS_CAUCHY) return 1.0 / (1.0 + s / a.lc2);
    else return 1.0;
}
// THE weighted linearisation of one observation at p: A, B and r, each multiplied by sqrt(w) once; with the squared loss no multiplication is made
template <int LOSS, int NA>
__device__ __forceinline__ void ba_linearise(const BaArgs& a, const double* P, const double* cam, const double (&p)[3], const float* kp, double (&A0)[NA], double (&A1)[NA],
                                             double (&B0)[3], double (&B1)[3], double& rx, double& ry) {
    ba_jacobians(P, cam, p, A0, A1, B0, B1);
    ba_residual(cam, p, kp, rx, ry);
    if constexpr (LOSS != LG_BA_LOSS_SQUARED) {
        const double sw = sqrt(ba_weight<LOSS>(a, rx * rx + ry * ry));
#pragma unroll
        for (int e = 0; e < NA; ++e) { A0[e] = sw * A0[e]; A1[e] = sw * A1[e]; }
#pragma unroll
        for (int e = 0; e < 3; ++e) { B0[e] = sw * B0[e]; B1[e] = sw * B1[e]; }
        rx = sw * rx; ry = sw * ry;
    }
}

// ------------------------------------------------------------------ records
template <bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_init_kernel(BaArgsOf<FOCAL> a) {
    constexpr int D = BA_COLS<FOCAL>;
    const long long g = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    if (g == 0) { BaHead h{}; h.lambda = a.lambda0; *a.head = h; }
    if (g < a.images) {
        const int k = (int)g;
        const float* c = a.cameras + (long long)k * 4;
        const float* p = a.poses + (long long)k * 12;
        bool ok = camera_ok(c);
#pragma unroll
        for (int e = 0; e < 12; ++e) ok = ok && isfinite(p[e]);
        BaImage im{};
        im.ok = ok ? 1 : 0; im.constant = a.constant[k] ? 1 : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) im.cam[e] = (double)c[e];
        if constexpr (FOCAL) {
            im.cconstant = (a.cconstant && a.cconstant[k]) ? 1 : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { a.cam[(long long)k * 4 + e] = (double)c[e]; a.cam[((long long)a.images + k) * 4 + e] = (double)c[e]; }
        }
        a.rec[k] = im;
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const double v = ok ? (double)p[e] : 0.0;
            a.pose[(long long)k * 12 + e] = v; a.pose[((long long)a.images + k) * 12 + e] = v;
        }
#pragma unroll
        for (int e = 0; e < D; ++e) a.delta[(long long)k * D + e] = 0.0;
        a.icost[k] = 0.0;
        a.status[k] = ok ? LG_OK : LG_ERR_CAMERA;
    }
    if (g < a.tracks) {
        a.tcnt[g] = 0; a.tcur[g] = 0; a.toff[g] = 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) { const double v = (double)a.xyz[g * 3 + e]; a.X[g * 3 + e] = v; a.X[((long long)a.tracks + g) * 3 + e] = v; }
    }
}

// ------------------------------------------------------------------ candidates
// AGAIN (after a filter): a candidate is a node still in state 1, and no state is written
template <bool AGAIN> __global__ __launch_bounds__(BA_THREADS) void ba_count_kernel(BaArgs a) {
    const int v = blockIdx.x * BA_THREADS + threadIdx.x;
    if (v >= a.nodes) return;
    if constexpr (AGAIN) {
        if (a.node_state[v] == 1) atomicAdd(a.tcnt + a.track_id[v], 1);
        return;
    }
    const int k = v / a.n, i = v - k * a.n;
    int state = 0;
    const long long j = a.track_id[v];
    if (i < live_rows(a.num, k, a.n) && j >= 0 && j < a.tracks) {
        const double* X = ba_point(a, 0, (int)j);
        if (!a.rec[k].ok) state = 2;
        else if (!(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]))) state = 3;
        else {
            double p[3];
            ba_project(ba_pose(a, 0, k), X, p);
            state = p[2] > 0.0 ? 1 : 4;
        }
        if (state == 1) atomicAdd(a.tcnt + j, 1);
    }
    a.node_state[v] = (unsigned char)state;
}

// the lists of the adjusted tracks (lg_solver_steps.h): ONE workgroup scans; one lane per node fills (states 5 / 6, the image's count); one lane per track sorts
__global__ __launch_bounds__(BA_SCAN_THREADS) void ba_scan_kernel(BaArgs a) {
    __shared__ int sh[BA_SCAN_WAVES];
    track_scan<BA_SCAN_THREADS>(a, sh);
}
__global__ __launch_bounds__(BA_THREADS) void ba_fill_kernel(BaArgs a) {
    const int v = blockIdx.x * BA_THREADS + threadIdx.x;
    if (track_fill<5, 6>(a, v)) atomicAdd(&a.rec[v / a.n].nact, 1);
}
__global__ __launch_bounds__(BA_THREADS) void ba_sort_kernel(BaArgs a) { track_sort(a, blockIdx.x * BA_THREADS + threadIdx.x); }

// ------------------------------------------------------------------ between two stages (lg_bundle_adjust_robust): the filter, then count<true>, scan, fill, sort, cost
// One lane per node: an active observation whose error at the accepted state exceeds the bar becomes state 7, counted by an integer atomicAdd.  The same
// launch, one lane per track and image: what moved so far is remembered (a track or image that stops moving returns its last accepted state), the trial point
// takes the accepted one (nothing writes a track's trial once it is not adjusted, and a later accepted step flips sel), and the counters the rebuild fills are
// cleared.  The node lanes read neither tcnt nor nact, so the order of the lanes does not matter
template <bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_filter_kernel(BaArgsOf<FOCAL> a, int first) {
    const long long g = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    const int s = a.head->sel;
    if (g < a.nodes && a.node_state[g] == 1) {
        const int k = (int)(g / a.n);
        double p[3], rx, ry;
        ba_project(ba_pose(a, s, k), ba_point(a, s, (int)a.track_id[g]), p);
        ba_residual(ba_cam<FOCAL>(a, s, k), p, a.kpts + g * 2, rx, ry);
        if (rx * rx + ry * ry > a.fe2) { a.node_state[g] = 7; atomicAdd(&a.head->removed, 1); }
    }
    if (g < a.tracks) {
        a.tmov[g] = ((first ? 0 : a.tmov[g]) || track_listed(a, (int)g)) ? 1 : 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) a.X[((long long)(s ^ 1) * a.tracks + g) * 3 + e] = a.X[((long long)s * a.tracks + g) * 3 + e];
        a.tcnt[g] = 0; a.tcur[g] = 0; a.toff[g] = 0;
    }
    if (g < a.images) {
        if (ba_free(a, (int)g)) a.rec[g].moved = 1;
        if constexpr (FOCAL) if (ba_cam_free(a, (int)g)) a.rec[g].cmoved = 1;
        a.rec[g].nact = 0;
    }
}

// one lane: if the filter removed something, the cost of the new set (the images' costs in ascending order), lambda and `converged` start again
__global__ void ba_restage_kernel(BaArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    BaHead& h = *a.head;
    if (h.removed > 0) {
        double sum = 0.0;
        int nobs = 0;
        for (int k = 0; k < a.images; ++k) { sum += a.icost[k]; nobs += a.rec[k].nact; }
        h.cost = sum; h.nobs = nobs; h.lambda = a.lambda0; h.converged = 0;
        h.filtered += h.removed; h.fstages += 1;
    }
    h.removed = 0; h.fail = 0;
}

// ------------------------------------------------------------------ the cost of a state: one workgroup per image, rows in ascending order
// trial = 0: the accepted state (the input); 1: the trial.  A row with pz <= 0 or a non-finite term fails the trial
template <int LOSS, bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_cost_kernel(BaArgsOf<FOCAL> a, int trial) {
    __shared__ double term[BA_THREADS];
    if (trial && a.head->converged) return;
    const int k = blockIdx.x, which = a.head->sel ^ trial;
    const double* P = ba_pose(a, which, k);
    const double* cam = ba_cam<FOCAL>(a, which, k);
    double sum = 0.0;
    int bad = 0;
    for (int i0 = 0; i0 < a.n; i0 += BA_THREADS) {
        const int i = i0 + threadIdx.x;
        double c = 0.0;
        if (i < a.n && a.node_state[(long long)k * a.n + i] == 1) {
            const long long v = (long long)k * a.n + i;
            double p[3], rx, ry;
            ba_project(P, ba_point(a, which, (int)a.track_id[v]), p);
            ba_residual(cam, p, a.kpts + v * 2, rx, ry);
            c = rx * rx + ry * ry;
            if (!(p[2] > 0.0) || !isfinite(c)) { bad = 1; c = 0.0; }
            if constexpr (LOSS != LG_BA_LOSS_SQUARED) c = ba_rho<LOSS>(a, c);      // rho(0) = 0
        }
        __syncthreads();
        term[threadIdx.x] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(BA_THREADS, a.n - i0);
            for (int q = 0; q < m; ++q) sum += term[q];
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        a.icost[k] = sum;
        if (bad) atomicOr(&a.head->fail, 1);
    }
}

// one lane: the images' costs in ascending order, the decision, lambda, the counters
__global__ void ba_decide_kernel(BaArgs a, int initial) {
    if (blockIdx.x || threadIdx.x) return;
    BaHead& h = *a.head;
    if (!initial && h.converged) return;
    double sum = 0.0;
    for (int k = 0; k < a.images; ++k) sum += a.icost[k];
    if (initial) {
        int nobs = 0;
        for (int k = 0; k < a.images; ++k) nobs += a.rec[k].nact;
        h.cost = sum; h.initial_cost = sum; h.nobs = nobs; h.fail = 0;
        return;
    }
    h.cost_new = sum;
    h.iters += 1;
    const bool ok = !h.fail && isfinite(sum);
    const bool conv = ok && fabs(h.cost - sum) <= a.ftol * h.cost, accept = ok && sum < h.cost;
    if (accept) { h.cost = sum; h.sel ^= 1; h.accepted += 1; h.lambda = fmax(h.lambda / 10.0, 1e-12); }
    else h.lambda = fmin(10.0 * h.lambda, 1e12);
    if (conv) h.converged = 1;
    h.fail = 0;
}

// ------------------------------------------------------------------ per iteration 1: one lane per track: V, g, the damped inverse, y
template <int LOSS, bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_points_kernel(BaArgsOf<FOCAL> a) {
    if (a.head->converged) return;
    const int j = blockIdx.x * BA_THREADS + threadIdx.x;
    if (j >= a.tracks || !track_listed(a, j)) return;
    const int s = a.head->sel, len = a.tcnt[j], off = a.toff[j];
    const double lambda = a.head->lambda;
    const double* Xp = ba_point(a, s, j);
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double V[6] = {0, 0, 0, 0, 0, 0}, G[3] = {0, 0, 0};
    for (int q = 0; q < len; ++q) {
        const int v = a.list[off + q], k = a.limg[off + q];
        const double* P = ba_pose(a, s, k);
        const double* cam = ba_cam<FOCAL>(a, s, k);
        double p[3], A0[6], A1[6], B0[3], B1[3], rx, ry;
        ba_project(P, X, p);
        ba_linearise<LOSS>(a, P, cam, p, a.kpts + (long long)v * 2, A0, A1, B0, B1, rx, ry);
        V[0] += B0[0] * B0[0] + B1[0] * B1[0]; V[1] += B0[0] * B0[1] + B1[0] * B1[1]; V[2] += B0[0] * B0[2] + B1[0] * B1[2];
        V[3] += B0[1] * B0[1] + B1[1] * B1[1]; V[4] += B0[1] * B0[2] + B1[1] * B1[2]; V[5] += B0[2] * B0[2] + B1[2] * B1[2];
#pragma unroll
        for (int e = 0; e < 3; ++e) G[e] += B0[e] * rx + B1[e] * ry;
    }
    V[0] = ba_damped(V[0], lambda); V[3] = ba_damped(V[3], lambda); V[5] = ba_damped(V[5], lambda);
    double Vi[3][3];
    const bool ok = tri_inverse3(V, Vi);
    double* vo = a.Vinv + (long long)j * 9;
    double* yo = a.y + (long long)j * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vo[3 * r + c] = ok ? Vi[r][c] : 0.0;
        yo[r] = ok ? (Vi[r][0] * G[0] + Vi[r][1] * G[1]) + Vi[r][2] * G[2] : 0.0;
    }
    if (!ok) atomicOr(&a.head->fail, 1);
}

// ------------------------------------------------------------------ per iteration 2: the block row of image a, BA_BCHUNK column blocks per workgroup
// grid (images, ceil(images / BA_BCHUNK)).  Threads 0 .. 215: entry (r, c) of block (a, b); in the workgroup that holds the diagonal block, threads 216 .. 248:
// the 21 entries of U_a's upper triangle, g_a (6), the sum of W y (6).  BA_TILE rows of image a at a time go through LDS in four steps: the first BA_TILE
// threads stage a row each (Y, A, r, W y, X, the row's track list); all threads count the list's entries per column block (integer LDS atomics: a count has no
// order); one thread per (row, column block) with an entry forms W_b once; then every entry thread adds its rows in ascending order.
// With a robust loss W_b carries the weight of ITS observation: the counting also finds the track's first entry in image b (an integer minimum), whose W goes
// to LDS; where a track has more than one observation in image b (rare) the entry threads form every W themselves, in the list's order
template <int LOSS, bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_reduce_kernel(BaArgsOf<FOCAL> a) {
    constexpr bool ROBUST = LOSS != LG_BA_LOSS_SQUARED;
    constexpr int D = BA_COLS<FOCAL>, DD = D * D, BCH = BA_CHUNK<FOCAL>, NU = D * (D + 1) / 2, NX = NU + 2 * D;     // columns per image, entries per block, column blocks, U's triangle, extras
    static_assert(DD * BCH + NX <= BA_THREADS, "entry threads and extras");
    __shared__ double sY[BA_TILE][3 * D], sA[BA_TILE][2 * D], sWy[BA_TILE][D], sX[BA_TILE][3], sR[BA_TILE][2], sW[BA_TILE][BCH][3 * D], sU[NX];
    __shared__ int sOff[BA_TILE], sLen[BA_TILE], sCnt[BA_TILE][BCH], sFirst[ROBUST ? BA_TILE : 1][BCH];
    if (a.head->converged) return;
    const int ia = blockIdx.x, b0 = blockIdx.y * BCH, t = threadIdx.x, dim = a.dim;
    if (b0 > ia) return;
    const bool diag = ia / BCH == (int)blockIdx.y, free_a = ba_any_free<FOCAL>(a, ia);
    const int bl = t / DD, rc = t - bl * DD, r = rc / D, c = rc - r * D, ib = b0 + bl;
    const bool entry = t < DD * BCH && ib <= ia;      // ib <= ia < images
    const int e = t - DD * BCH;                             // 0 .. NX - 1 in the diagonal workgroup: U (21 | 28), g (D), W y (D)
    const bool extra = diag && e >= 0 && e < NX;
    double* out = a.S + ((long long)(D * ia + r) * dim + D * ib + c);
    if (!free_a) {                                          // the image's columns drop out: identity, zero coupling, zero right-hand side
        if (entry) *out = (ib == ia && r == c) ? 1.0 : 0.0;
        if (extra && e >= NU + D) a.S[(long long)dim * dim + D * ia + (e - (NU + D))] = 0.0;
        return;
    }
    const int s = a.head->sel;
    const double lambda = a.head->lambda;
    const bool free_b = entry && ba_any_free<FOCAL>(a, ib);
    // the thread's (row, column block) item of a tile, and the pose of that block's image
    const int iq = t / BCH, ibl = t - iq * BCH, item_b = b0 + ibl;
    const bool item = t < BA_TILE * BCH, item_free = item && item_b <= ia && ba_any_free<FOCAL>(a, item_b);
    double Pb[12], fb[ROBUST ? 4 : 2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 12; ++q) Pb[q] = item_free ? ba_pose(a, s, item_b)[q] : 0.0;
    if (item_free) { fb[0] = ba_cam<FOCAL>(a, s, item_b)[0]; fb[1] = ba_cam<FOCAL>(a, s, item_b)[1]; }
    if constexpr (ROBUST) if (item_free) { fb[2] = ba_cam<FOCAL>(a, s, item_b)[2]; fb[3] = ba_cam<FOCAL>(a, s, item_b)[3]; }
    const int cq = t >> 3, part = t & 7;                    // counting: 8 threads per row of the tile
    static_assert(BA_THREADS == 8 * BA_TILE && BA_TILE * BCH <= BA_THREADS, "8 counting threads and BCH items per tile row");
    // U's upper triangle in row-major order: entry e -> (ur, uc)
    int ur = 0, uc = 0;
    if (extra && e < NU) { int left = e; while (left >= D - ur) { left -= D - ur; ++ur; } uc = ur + left; }
    const double* Pa = ba_pose(a, s, ia);
    const double* cama = ba_cam<FOCAL>(a, s, ia);
    double acc = 0.0;
    for (int i0 = 0; i0 < a.n; i0 += BA_TILE) {
        __syncthreads();                                    // the previous tile has been read
        if (t < BA_TILE) {
            const int i = i0 + t;
            const long long v = (long long)ia * a.n + i;
            int len = 0;
            if (i < a.n && a.node_state[v] == 1) {
                const int j = (int)a.track_id[v];
                len = a.tcnt[j]; sOff[t] = a.toff[j];
                const double* Xp = ba_point(a, s, j);
                const double* Vi = a.Vinv + (long long)j * 9;
                const double* y = a.y + (long long)j * 3;
                double p[3], A0[D], A1[D], B0[3], B1[3], rx, ry;
                ba_project(Pa, Xp, p);
                // squared: ba_linearise<0>'s two calls written out; through the wrapper the compiler allocates this kernel's registers differently from
                // lg_bundle_adjust's build before the robust mode (measured: 0.9 % on a call, profiles/bundle_adjust_robust.md): like this the instruction stream is that one
                if constexpr (ROBUST) ba_linearise<LOSS>(a, Pa, cama, p, a.kpts + v * 2, A0, A1, B0, B1, rx, ry);
                else { ba_jacobians(Pa, cama, p, A0, A1, B0, B1); ba_residual(cama, p, a.kpts + v * 2, rx, ry); }
                sX[t][0] = Xp[0]; sX[t][1] = Xp[1]; sX[t][2] = Xp[2];
                sR[t][0] = rx; sR[t][1] = ry;
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    sA[t][q] = A0[q]; sA[t][D + q] = A1[q];
                    const double w0 = A0[q] * B0[0] + A1[q] * B1[0], w1 = A0[q] * B0[1] + A1[q] * B1[1], w2 = A0[q] * B0[2] + A1[q] * B1[2];
#pragma unroll
                    for (int m = 0; m < 3; ++m) sY[t][3 * q + m] = (w0 * Vi[m] + w1 * Vi[3 + m]) + w2 * Vi[6 + m];
                    sWy[t][q] = (w0 * y[0] + w1 * y[1]) + w2 * y[2];
                }
            }
            sLen[t] = len;
        }
        if (item) sCnt[iq][ibl] = 0;
        if constexpr (ROBUST) if (item) sFirst[iq][ibl] = 0x7FFFFFFF;
        __syncthreads();
        {
            const int len = sLen[cq], off = sOff[cq];
            for (int l = part; l < len; l += 8) {
                const int d = a.limg[off + l] - b0;
                if (d >= 0 && d < BCH && b0 + d <= ia) {
                    atomicAdd(&sCnt[cq][d], 1);
                    if constexpr (ROBUST) atomicMin(&sFirst[cq][d], l);
                }
            }
        }
        __syncthreads();
        if (item_free && sCnt[iq][ibl] > 0) {               // W of (image item_b, the row's track): it does not depend on the observation's row in b
            double p[3], A0[D], A1[D], B0[3], B1[3];
            ba_project(Pb, sX[iq], p);
            if constexpr (ROBUST) {                             // the weight of the track's first observation in image item_b (sCnt > 0: sFirst < sLen)
                double rx, ry;
                ba_linearise<LOSS>(a, Pb, fb, p, a.kpts + (long long)a.list[sOff[iq] + sFirst[iq][ibl]] * 2, A0, A1, B0, B1, rx, ry);
            } else ba_jacobians(Pb, fb, p, A0, A1, B0, B1);
#pragma unroll
            for (int q = 0; q < D; ++q)
#pragma unroll
                for (int m = 0; m < 3; ++m) sW[iq][ibl][3 * q + m] = A0[q] * B0[m] + A1[q] * B1[m];
        }
        __syncthreads();
        const int rows = min(BA_TILE, a.n - i0);
        if (free_b) {
            for (int q = 0; q < rows; ++q) {
                const int times = sCnt[q][bl];              // the observations of the row's track in image b, in order: the same W each
                if (!times) continue;
                if constexpr (ROBUST) if (times > 1) {          // every observation of the row's track in image ib has a weight of its own
                    const double* Pi = ba_pose(a, s, ib);
                    const double* cami = ba_cam<FOCAL>(a, s, ib);
                    for (int l = 0; l < sLen[q]; ++l) {
                        if (a.limg[sOff[q] + l] != ib) continue;
                        double p[3], A0[D], A1[D], B0[3], B1[3], rx, ry, a0 = 0.0, a1 = 0.0;
                        ba_project(Pi, sX[q], p);
                        ba_linearise<LOSS>(a, Pi, cami, p, a.kpts + (long long)a.list[sOff[q] + l] * 2, A0, A1, B0, B1, rx, ry);
#pragma unroll
                        for (int cc = 0; cc < D; ++cc) if (cc == c) { a0 = A0[cc]; a1 = A1[cc]; }
                        acc += (sY[q][3 * r] * (a0 * B0[0] + a1 * B1[0]) + sY[q][3 * r + 1] * (a0 * B0[1] + a1 * B1[1])) + sY[q][3 * r + 2] * (a0 * B0[2] + a1 * B1[2]);
                    }
                    continue;
                }
                const double term = (sY[q][3 * r] * sW[q][bl][3 * c] + sY[q][3 * r + 1] * sW[q][bl][3 * c + 1]) + sY[q][3 * r + 2] * sW[q][bl][3 * c + 2];
                for (int m = 0; m < times; ++m) acc += term;
            }
        } else if (extra) {
            for (int q = 0; q < rows; ++q) {
                if (!sLen[q]) continue;
                if (e < NU) acc += sA[q][ur] * sA[q][uc] + sA[q][D + ur] * sA[q][D + uc];
                else if (e < NU + D) acc += sA[q][e - NU] * sR[q][0] + sA[q][D + e - NU] * sR[q][1];
                else acc += sWy[q][e - (NU + D)];
            }
        }
    }
    if (extra) sU[e] = acc;
    __syncthreads();
    if (entry) {
        double val = free_b ? -acc : 0.0;
        if (ib == ia) {                                     // the diagonal block: U' - E (this workgroup is the diagonal one, sU is its own)
            const int lo = min(r, c), hi = max(r, c);
            double u = sU[lo * D - lo * (lo - 1) / 2 + (hi - lo)];
            if (r == c) u = ba_damped(u, lambda);
            val = u - acc;
        }
        if constexpr (FOCAL)                                // a held column of either image: identity, zero coupling
            if (!((r < 6 ? ba_free(a, ia) : ba_cam_free(a, ia)) && (c < 6 ? ba_free(a, ib) : ba_cam_free(a, ib)))) val = (ib == ia && r == c) ? 1.0 : 0.0;
        *out = val;
    }
    if (extra && e >= NU + D) {                             // (sum of W y) - g
        double rhs = acc - sU[e - D];
        if constexpr (FOCAL) if (!(e - (NU + D) < 6 ? ba_free(a, ia) : ba_cam_free(a, ia))) rhs = 0.0;
        a.S[(long long)dim * dim + D * ia + (e - (NU + D))] = rhs;
    }
}

// ------------------------------------------------------------------ per iteration 3: panel p of the left-looking blocked Cholesky, the right-hand side as row dim
// Two launches per panel, so that no workgroup reads what another workgroup of its launch writes.  Thread (tr, tc) of the 16 x 16 grid holds entries
// (tr + 16 ii, tc + 16 jj), ii, jj < 3, of a BA_NB x BA_NB block.
// 3a. ONE workgroup: the panel's diagonal block D = S_pp - L_p L_p^T over all earlier columns, factored in LDS and written over S_pp
__global__ __launch_bounds__(BA_THREADS) void ba_cholesky_diag_kernel(BaArgs a, int panel) {
    __shared__ CholeskyDiagLds m;
    if (a.head->converged) return;
    cholesky_diag(a.S, a.dim, panel, 0.0, &a.head->fail, m);            // floor 0: a pivot fails unless it is > 0 (and finite)
}

// 3b. one workgroup per BA_NB-row tile that has rows below the diagonal block: G = S_ip - L_i L_p^T, then L_i = G L_pp^-T.  It reads the panel's rows (earlier
// columns and L_pp: finished by earlier launches) and its own rows; it writes its own rows' panel columns, which no other workgroup of the launch reads
__global__ __launch_bounds__(BA_THREADS) void ba_cholesky_rows_kernel(BaArgs a, int panel) {
    __shared__ CholeskyRowsLds m;
    if (a.head->converged) return;
    cholesky_rows(a.S, a.dim, 1, panel, panel + blockIdx.x, m);
}

// ------------------------------------------------------------------ per iteration 4: ONE workgroup: L^T s = z backwards, the trial poses
// FOCAL: 7 entries per image, and the trial cameras, f <- f exp(d) for fx and fy of a free camera (a trial focal length that is not finite or not > 0 fails
// the step); a held column's step is 0
template <bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_backsolve_kernel(BaArgsOf<FOCAL> a) {
    constexpr int D = BA_COLS<FOCAL>;
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
        if constexpr (FOCAL) {
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
        }
        if (!ba_free(a, k)) {
            for (int q = 0; q < 12; ++q) out[q] = P[q];
            for (int q = 0; q < 6; ++q) a.delta[k * D + q] = 0.0;
            continue;
        }
        double x[6], Q[9];
#pragma unroll
        for (int q = 0; q < 6; ++q) { x[q] = sd[D * k + q]; a.delta[k * D + q] = x[q]; }
        so3_exp(x, Q);
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

// ------------------------------------------------------------------ per iteration 5: one lane per track: the point's step and its trial
template <int LOSS, bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_trial_points_kernel(BaArgsOf<FOCAL> a) {
    constexpr int D = BA_COLS<FOCAL>;              // a held column's step is 0 (ba_backsolve)
    if (a.head->converged) return;
    const int j = blockIdx.x * BA_THREADS + threadIdx.x;
    if (j >= a.tracks || !track_listed(a, j)) return;
    const int s = a.head->sel, len = a.tcnt[j], off = a.toff[j];
    const double* Xp = ba_point(a, s, j);
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < len; ++q) {
        const int k = a.limg[off + q];
        if (!ba_any_free<FOCAL>(a, k)) continue;
        const double* P = ba_pose(a, s, k);
        const double* d = a.delta + (long long)k * D;
        double p[3], A0[D], A1[D], B0[3], B1[3], rx, ry;       // the squared loss reads neither the residual nor the keypoint
        ba_project(P, X, p);
        ba_linearise<LOSS>(a, P, ba_cam<FOCAL>(a, s, k), p, a.kpts + (long long)a.list[off + q] * 2, A0, A1, B0, B1, rx, ry);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            double w = 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) w += (A0[r] * B0[m] + A1[r] * B1[m]) * d[r];
            acc[m] += w;
        }
    }
    const double* Vi = a.Vinv + (long long)j * 9;
    const double* y = a.y + (long long)j * 3;
    double* out = a.X + ((long long)(s ^ 1) * a.tracks + j) * 3;
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double v = X[r] - (y[r] + ((Vi[3 * r] * acc[0] + Vi[3 * r + 1] * acc[1]) + Vi[3 * r + 2] * acc[2]));
        fin = fin && isfinite(v);
        out[r] = v;
    }
    if (!fin) atomicOr(&a.head->fail, 1);
}

// ------------------------------------------------------------------ lg_bundle_adjust_pcg: the reduced camera system solved by preconditioned conjugate gradients
// S is never formed: per solver iteration q = S p is one pass over the tracks (u = Vi sum of W^T p) and one over the images (q = U' p - sum of W u), and ONE
// workgroup does the two dot products, alpha, beta and the vector updates.  Every launch of the whole budget is enqueued; the step kernel alone writes
// BaPcgHead (the call's first setup launch clears it), and once `done` names the running Levenberg-Marquardt iteration (or the trial has failed, or the call converged) the rest return at once.
// The bodies of the trial pose and of the track's sum of W^T p stand here a second time, next to ba_backsolve_kernel's and ba_trial_points_kernel's: called
// from those kernels as shared device functions they changed the kernels' instruction streams, which this file keeps (profiles/bundle_adjust_pcg.md)
constexpr int PCG_THREADS = 64, PCG_STEP_THREADS = 1024, PCG_PARTIALS = IMAGE_SUM_PARTIALS;      // setup and images: one wave per image, a tile is 64 rows; the dots: image_sum (lg_solver_steps.h)
constexpr int PCG_NT = 21, PCG_SUMS = 2 * PCG_NT + 12;                               // E_aa's lower triangle, U's upper triangle, g, the sum of W y

struct BaPcgHead { double rz, rz0; int done, cg_total, unconverged, pad; };          // done: 1 + the Levenberg-Marquardt iteration (counted over the call) whose solve ended
static_assert(sizeof(BaPcgHead) <= 256, "the record of the solver is 256 bytes");
struct BaPcgArgs : BaArgs {
    BaPcgHead* ph; double* r; double* z; double* p; double* q; double* U; double* M; double* pq; double* rz; double* u;      // x is `delta`; U, M [images][36]; u [tracks][3]
    double tol; int budget;
};

// entry r of (6 x 6 row-major) m times v: the products over c ascending, the first starts the sum
__device__ __forceinline__ double pcg_row(const double* m, int r, const double (&v)[6]) {
    double s = m[6 * r] * v[0];
#pragma unroll
    for (int c = 1; c < 6; ++c) s += m[6 * r + c] * v[c];
    return s;
}
__device__ __forceinline__ double pcg_dot6(const double (&x)[6], const double (&y)[6]) {
    double s = x[0] * y[0];
#pragma unroll
    for (int e = 1; e < 6; ++e) s += x[e] * y[e];
    return s;
}

// one workgroup (one wave) per image: U', b, M = S_aa^-1 and the start of the solve (x = 0, r = b, z = M b, p = z, the image's r.z).  A tile of 64 rows at a
// time: lane t linearises row t (A, r, W, Y = W Vi, W y, how often the row's track is seen in this image) into LDS, then lane e < 54 adds its entry over the
// tile's active rows in ascending order.  E_aa as in ba_reduce_kernel: the row's own W once per observation of its track in the image with the squared
// loss; with a robust loss every such observation's own W, formed by the entry lanes (rare)
template <int LOSS> __global__ __launch_bounds__(PCG_THREADS) void ba_pcg_setup_kernel(BaPcgArgs a, int lm) {
    constexpr bool ROBUST = LOSS != LG_BA_LOSS_SQUARED;
    __shared__ double sA[PCG_THREADS][12], sR[PCG_THREADS][2], sWy[PCG_THREADS][6], sY[PCG_THREADS][18], sW[PCG_THREADS][18], sX[PCG_THREADS][3], sS[PCG_SUMS], sL[PCG_NT], sM[36], sV[12];
    __shared__ int sCnt[PCG_THREADS], sOff[PCG_THREADS], sLen[PCG_THREADS];
    const int ia = blockIdx.x, t = threadIdx.x;
    if (lm == 0 && ia == 0 && t == 0) *a.ph = BaPcgHead{};   // the call's first solver launch clears the record (no launch of this one reads it)
    if (a.head->converged) return;
    const long long at = (long long)ia * 6;
    if (!ba_free(a, ia)) {                                  // no unknowns: every entry is 0
        if (t < 6) { a.delta[at + t] = 0.0; a.r[at + t] = 0.0; a.z[at + t] = 0.0; a.p[at + t] = 0.0; a.q[at + t] = 0.0; }
        if (t == 0) { a.pq[ia] = 0.0; a.rz[ia] = 0.0; }
        return;
    }
    const int s = a.head->sel;
    const double lambda = a.head->lambda;
    const double* Pa = ba_pose(a, s, ia);
    const double* cama = a.rec[ia].cam;
    // lane e: 0 .. 20 entry (er, ec), ec <= er, of E_aa (row-major lower triangle); 21 .. 41 entry (er, ec), er <= ec, of U (row-major upper triangle);
    // 42 .. 47 g; 48 .. 53 the sum of W y
    int er = 0, ec = 0;
    if (t < PCG_NT) { int left = t; while (left > er) { left -= er + 1; ++er; } ec = left; }
    else if (t < 2 * PCG_NT) { int left = t - PCG_NT; while (left >= 6 - er) { left -= 6 - er; ++er; } ec = er + left; }
    double acc = 0.0;
    for (int i0 = 0; i0 < a.n; i0 += PCG_THREADS) {
        __syncthreads();                                    // the previous tile has been read
        const int i = i0 + t;
        const long long v = (long long)ia * a.n + i;
        int cnt = 0;
        if (i < a.n && a.node_state[v] == 1) {
            const int j = (int)a.track_id[v], len = a.tcnt[j], off = a.toff[j];
            const double* Xp = ba_point(a, s, j);
            const double* Vi = a.Vinv + (long long)j * 9;
            const double* y = a.y + (long long)j * 3;
            double p[3], A0[6], A1[6], B0[3], B1[3], rx, ry;
            ba_project(Pa, Xp, p);
            ba_linearise<LOSS>(a, Pa, cama, p, a.kpts + v * 2, A0, A1, B0, B1, rx, ry);
            sX[t][0] = Xp[0]; sX[t][1] = Xp[1]; sX[t][2] = Xp[2];
            sR[t][0] = rx; sR[t][1] = ry;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                sA[t][q] = A0[q]; sA[t][6 + q] = A1[q];
                const double w0 = A0[q] * B0[0] + A1[q] * B1[0], w1 = A0[q] * B0[1] + A1[q] * B1[1], w2 = A0[q] * B0[2] + A1[q] * B1[2];
                sW[t][3 * q] = w0; sW[t][3 * q + 1] = w1; sW[t][3 * q + 2] = w2;
#pragma unroll
                for (int m = 0; m < 3; ++m) sY[t][3 * q + m] = (w0 * Vi[m] + w1 * Vi[3 + m]) + w2 * Vi[6 + m];
                sWy[t][q] = (w0 * y[0] + w1 * y[1]) + w2 * y[2];
            }
            for (int l = 0; l < len; ++l) cnt += a.limg[off + l] == ia ? 1 : 0;     // >= 1: the row itself
            sOff[t] = off; sLen[t] = len;
        }
        sCnt[t] = cnt;
        __syncthreads();
        if (t >= PCG_SUMS) continue;
        const int rows = min(PCG_THREADS, a.n - i0);
        for (int q = 0; q < rows; ++q) {
            const int times = sCnt[q];
            if (!times) continue;
            if (t < PCG_NT) {
                if constexpr (ROBUST) if (times > 1) {      // every observation of the row's track in this image has a weight of its own
                    for (int l = 0; l < sLen[q]; ++l) {
                        if (a.limg[sOff[q] + l] != ia) continue;
                        double p[3], A0[6], A1[6], B0[3], B1[3], rx, ry, a0 = 0.0, a1 = 0.0;
                        ba_project(Pa, sX[q], p);
                        ba_linearise<LOSS>(a, Pa, cama, p, a.kpts + (long long)a.list[sOff[q] + l] * 2, A0, A1, B0, B1, rx, ry);
#pragma unroll
                        for (int cc = 0; cc < 6; ++cc) if (cc == ec) { a0 = A0[cc]; a1 = A1[cc]; }
                        acc += (sY[q][3 * er] * (a0 * B0[0] + a1 * B1[0]) + sY[q][3 * er + 1] * (a0 * B0[1] + a1 * B1[1])) + sY[q][3 * er + 2] * (a0 * B0[2] + a1 * B1[2]);
                    }
                    continue;
                }
                const double term = (sY[q][3 * er] * sW[q][3 * ec] + sY[q][3 * er + 1] * sW[q][3 * ec + 1]) + sY[q][3 * er + 2] * sW[q][3 * ec + 2];
                for (int m = 0; m < times; ++m) acc += term;
            } else if (t < 2 * PCG_NT) acc += sA[q][er] * sA[q][ec] + sA[q][6 + er] * sA[q][6 + ec];
            else if (t < 2 * PCG_NT + 6) acc += sA[q][t - 2 * PCG_NT] * sR[q][0] + sA[q][6 + t - 2 * PCG_NT] * sR[q][1];
            else acc += sWy[q][t - (2 * PCG_NT + 6)];
        }
    }
    if (t < PCG_SUMS) sS[t] = acc;
    __syncthreads();
    // U' (mirrored, its diagonal damped) and b = (sum of W y) - g
    if (t < 36) {
        const int r = t / 6, c = t - 6 * r, lo = min(r, c), hi = max(r, c);
        double u = sS[PCG_NT + lo * 6 - lo * (lo - 1) / 2 + (hi - lo)];
        if (r == c) u = ba_damped(u, lambda);
        a.U[(long long)ia * 36 + t] = u;
    }
    if (t < 6) sV[t] = sS[2 * PCG_NT + 6 + t] - sS[2 * PCG_NT + t];
    // lane 0: S_aa = U' - E_aa = L L^T by rows, in registers; a pivot that is not > 0 (or not finite) fails the trial and 1 takes its place
    if (t == 0) {
        double L[PCG_NT];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double u = sS[PCG_NT + j * 6 - j * (j - 1) / 2 + (i - j)];
                if (i == j) u = ba_damped(u, lambda);
                double d = u - sS[i * (i + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; ++k) d = d - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
                if (i == j) {
                    if (!(isfinite(d) && d > 0.0)) { bad = true; d = 1.0; }
                    L[i * (i + 1) / 2 + j] = sqrt(d);
                } else L[i * (i + 1) / 2 + j] = d / L[j * (j + 1) / 2 + j];
            }
#pragma unroll
        for (int e = 0; e < PCG_NT; ++e) sL[e] = L[e];
        if (bad) atomicOr(&a.head->fail, 1);
    }
    __syncthreads();
    // lane c < 6: column c of M = S_aa^-1: L w = e_c forwards, L^T m = w backwards
    if (t < 6) {
        double w[6], m[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double d = i == t ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) d = d - sL[i * (i + 1) / 2 + k] * w[k];
            w[i] = d / sL[i * (i + 1) / 2 + i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double d = w[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) d = d - sL[k * (k + 1) / 2 + i] * m[k];
            m[i] = d / sL[i * (i + 1) / 2 + i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) { a.M[(long long)ia * 36 + 6 * i + t] = m[i]; sM[6 * i + t] = m[i]; }
    }
    __syncthreads();
    if (t < 6) {
        double b[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) b[e] = sV[e];
        const double zr = pcg_row(sM, t, b);
        a.delta[at + t] = 0.0; a.r[at + t] = b[t]; a.z[at + t] = zr; a.p[at + t] = zr; a.q[at + t] = 0.0;
        sV[6 + t] = zr;
    }
    __syncthreads();
    if (t == 0) {
        double b[6], z[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) { b[e] = sV[e]; z[e] = sV[6 + e]; }
        a.rz[ia] = pcg_dot6(b, z); a.pq[ia] = 0.0;
    }
}

// the solve of Levenberg-Marquardt iteration `lm` (counted over the call) is over, or not to be run
__device__ __forceinline__ bool pcg_idle(const BaPcgArgs& a, int lm) { return a.head->converged || a.head->fail || a.ph->done == lm + 1; }

// one lane per listed track: u = Vi sum of W^T p (ba_trial_points_kernel's sum with p in place of the step)
template <int LOSS> __global__ __launch_bounds__(BA_THREADS) void ba_pcg_tracks_kernel(BaPcgArgs a, int lm) {
    if (pcg_idle(a, lm)) return;
    const int j = blockIdx.x * BA_THREADS + threadIdx.x;
    if (j >= a.tracks || !track_listed(a, j)) return;
    const int s = a.head->sel, len = a.tcnt[j], off = a.toff[j];
    const double* Xp = ba_point(a, s, j);
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < len; ++q) {
        const int k = a.limg[off + q];
        if (!ba_free(a, k)) continue;
        const double* P = ba_pose(a, s, k);
        const double* d = a.p + (long long)k * 6;
        double p[3], A0[6], A1[6], B0[3], B1[3], rx, ry;
        ba_project(P, X, p);
        ba_linearise<LOSS>(a, P, a.rec[k].cam, p, a.kpts + (long long)a.list[off + q] * 2, A0, A1, B0, B1, rx, ry);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            double w = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) w += (A0[r] * B0[m] + A1[r] * B1[m]) * d[r];
            acc[m] += w;
        }
    }
    const double* Vi = a.Vinv + (long long)j * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) a.u[(long long)j * 3 + r] = (Vi[3 * r] * acc[0] + Vi[3 * r + 1] * acc[1]) + Vi[3 * r + 2] * acc[2];
}

// one workgroup (one wave) per image: q = U' p - sum of W u over its active rows in ascending row order, and the image's p.q.  Lane t forms W u of row t of a
// tile; lanes 0 .. 5 add their entry over the tile's active rows (the wave's ballot names them) in ascending order
template <int LOSS> __global__ __launch_bounds__(PCG_THREADS) void ba_pcg_images_kernel(BaPcgArgs a, int lm) {
    __shared__ double sT[PCG_THREADS][7], sQ[6];
    if (pcg_idle(a, lm)) return;                            // uniform over the grid: no launch between the step kernels writes any of the three
    const int ia = blockIdx.x, t = threadIdx.x;
    if (!ba_free(a, ia)) return;                            // q and the partial stay 0 (ba_pcg_setup_kernel)
    const int s = a.head->sel;
    const double* Pa = ba_pose(a, s, ia);
    const double* cama = a.rec[ia].cam;
    double acc = 0.0;
    for (int i0 = 0; i0 < a.n; i0 += PCG_THREADS) {
        __syncthreads();                                    // the previous tile has been read
        const int i = i0 + t;
        const long long v = (long long)ia * a.n + i;
        const bool active = i < a.n && a.node_state[v] == 1;
        if (active) {
            const int j = (int)a.track_id[v];
            const double* u = a.u + (long long)j * 3;
            double p[3], A0[6], A1[6], B0[3], B1[3], rx, ry;
            ba_project(Pa, ba_point(a, s, j), p);
            ba_linearise<LOSS>(a, Pa, cama, p, a.kpts + v * 2, A0, A1, B0, B1, rx, ry);
#pragma unroll
            for (int r = 0; r < 6; ++r)
                sT[t][r] = ((A0[r] * B0[0] + A1[r] * B1[0]) * u[0] + (A0[r] * B0[1] + A1[r] * B1[1]) * u[1]) + (A0[r] * B0[2] + A1[r] * B1[2]) * u[2];
        }
        unsigned long long mask = __ballot(active);
        __syncthreads();
        if (t < 6)
            while (mask) { const int q = __ffsll((long long)mask) - 1; mask &= mask - 1; acc += sT[q][t]; }
    }
    if (t < 6) {
        double p[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) p[e] = a.p[(long long)ia * 6 + e];
        const double qv = pcg_row(a.U + (long long)ia * 36, t, p) - acc;
        a.q[(long long)ia * 6 + t] = qv;
        sQ[t] = qv;
    }
    __syncthreads();
    if (t == 0) {
        double p[6], q[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) { p[e] = a.p[(long long)ia * 6 + e]; q[e] = sQ[e]; }
        a.pq[ia] = pcg_dot6(p, q);
    }
}

// ONE workgroup, solver iteration `it` of Levenberg-Marquardt iteration `lm`: p.q, alpha, x, r, z = M r, r.z, the stopping test, beta, p; the record; when the
// solve ends the trial poses (ba_backsolve_kernel's).  Strided loops over the images, no per-image LDS array
__global__ __launch_bounds__(PCG_STEP_THREADS) void ba_pcg_step_kernel(BaPcgArgs a, int lm, int it) {
    __shared__ double part[PCG_PARTIALS];
    const int t = threadIdx.x;
    BaPcgHead& h = *a.ph;
    if (pcg_idle(a, lm)) return;
    const int s = a.head->sel;
    double rz = h.rz, rz0 = h.rz0;                          // (read by all before lane 0 writes them again, behind the barriers of image_sum)
    bool end = false, bad = false;
    if (it == 0) {
        rz = rz0 = image_sum(a.rz, a.images, part);
        if (t == 0) { h.rz = rz; h.rz0 = rz0; }
        if (!(isfinite(rz) && rz >= 0.0)) bad = true;
        else if (rz == 0.0) end = true;                     // b = 0 (no free image among them): x = 0
    }
    double rz_new = rz;
    if (!bad && !end) {
        const double pq = image_sum(a.pq, a.images, part);
        if (!(isfinite(pq) && pq > 0.0)) bad = true;
        else {
            const double alpha = rz / pq;
            for (int k = t; k < a.images; k += PCG_STEP_THREADS) {
                if (!ba_free(a, k)) continue;
                const long long at = (long long)k * 6;
                double r[6], z[6];
#pragma unroll
                for (int e = 0; e < 6; ++e) {
                    a.delta[at + e] = a.delta[at + e] + alpha * a.p[at + e];
                    r[e] = a.r[at + e] - alpha * a.q[at + e];
                    a.r[at + e] = r[e];
                }
#pragma unroll
                for (int e = 0; e < 6; ++e) { z[e] = pcg_row(a.M + (long long)k * 36, e, r); a.z[at + e] = z[e]; }
                a.rz[k] = pcg_dot6(r, z);
            }
            rz_new = image_sum(a.rz, a.images, part);
            if (t == 0) h.cg_total += 1;
            if (!(isfinite(rz_new) && rz_new >= 0.0)) bad = true;
            else {
                const bool reached = sqrt(rz_new) <= a.tol * sqrt(rz0);
                end = reached || it == a.budget - 1;
                if (end && !reached && t == 0) h.unconverged += 1;
            }
        }
    }
    if (bad) { if (t == 0) atomicOr(&a.head->fail, 1); return; }
    if (!end) {
        const double beta = rz_new / rz;
        for (int k = t; k < a.images; k += PCG_STEP_THREADS) {
            if (!ba_free(a, k)) continue;
#pragma unroll
            for (int e = 0; e < 6; ++e) a.p[(long long)k * 6 + e] = a.z[(long long)k * 6 + e] + beta * a.p[(long long)k * 6 + e];
        }
        if (t == 0) h.rz = rz_new;
        return;
    }
    if (t == 0) h.done = lm + 1;
    int fail = 0;
    for (int k = t; k < a.images; k += PCG_STEP_THREADS) {
        const double* P = ba_pose(a, s, k);
        double* out = a.pose + ((long long)(s ^ 1) * a.images + k) * 12;
        if (!ba_free(a, k)) {
            for (int q = 0; q < 12; ++q) out[q] = P[q];
            continue;
        }
        double x[6], Q[9];
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = a.delta[(long long)k * 6 + q];
        so3_exp(x, Q);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = (Q[3 * i] * P[j] + Q[3 * i + 1] * P[4 + j]) + Q[3 * i + 2] * P[8 + j];
                if (j == 3) v = v + x[3 + i];
                if (!isfinite(v)) fail = 1;
                out[4 * i + j] = v;
            }
    }
    if (fail) atomicOr(&a.head->fail, 1);
}

// one lane, behind the scatter: the two counters of the solver
__global__ void ba_pcg_summary_kernel(BaPcgArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    a.summary[7] = (double)a.ph->cg_total; a.summary[11] = (double)a.ph->unconverged;
}

// ------------------------------------------------------------------ the outputs
// ROBUST (lg_bundle_adjust_robust): summary [12], and a track or image that moved in an earlier stage returns its last accepted state
// FOCAL (lg_bundle_adjust_focal): cameras_out, and summary [10] = the cameras that were free in any stage
template <bool ROBUST, bool FOCAL> __global__ __launch_bounds__(BA_THREADS) void ba_scatter_kernel(BaArgsOf<FOCAL> a) {
    const long long g = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    const BaHead h = *a.head;
    const int s = h.sel;
    if (g == 0) {
        a.summary[0] = h.initial_cost; a.summary[1] = h.cost; a.summary[2] = (double)h.iters; a.summary[3] = (double)h.accepted;
        a.summary[4] = (double)h.converged; a.summary[5] = (double)h.nobs; a.summary[6] = h.lambda; a.summary[7] = 0.0;
        if constexpr (ROBUST) { a.summary[8] = (double)h.filtered; a.summary[9] = (double)h.fstages; a.summary[10] = 0.0; a.summary[11] = 0.0; }
        if constexpr (FOCAL) {
            int moved = 0;
            for (int k = 0; k < a.images; ++k) moved += (ba_cam_free(a, k) || a.rec[k].cmoved) ? 1 : 0;
            a.summary[10] = (double)moved;
        }
    }
    if (g < a.nodes) {
        const int k = (int)(g / a.n);
        float x = __builtin_nanf(""), y = x, z = x, err = x;
        if (a.node_state[g] == 1) {
            const double* X = ba_point(a, s, (int)a.track_id[g]);
            double p[3], rx, ry;
            ba_project(ba_pose(a, s, k), X, p);
            ba_residual(ba_cam<FOCAL>(a, s, k), p, a.kpts + g * 2, rx, ry);
            x = (float)X[0]; y = (float)X[1]; z = (float)X[2]; err = (float)sqrt(rx * rx + ry * ry);
        }
        float* o = a.points3d + g * 3;
        o[0] = x; o[1] = y; o[2] = z;
        a.obs_err[g] = err;
    }
    if (g < a.tracks) {
        bool adj = track_listed(a, (int)g);
        if constexpr (ROBUST) adj = adj || (a.tmov && a.tmov[g]);
        const double* X = ba_point(a, s, (int)g);
#pragma unroll
        for (int e = 0; e < 3; ++e) a.xyz_out[g * 3 + e] = adj ? (float)X[e] : a.xyz[g * 3 + e];
    }
    if (g < a.images) {
        bool fr = ba_free(a, (int)g);
        if constexpr (ROBUST) fr = fr || a.rec[g].moved;
        const double* P = ba_pose(a, s, (int)g);
#pragma unroll
        for (int e = 0; e < 12; ++e) a.poses_out[g * 12 + e] = fr ? (float)P[e] : a.poses[g * 12 + e];
        if constexpr (FOCAL) {                              // fx, fy of a camera that moved; cx, cy and every other row are the input's bits
            const bool cf = ba_cam_free(a, (int)g) || a.rec[g].cmoved;
            const double* c = ba_cam<true>(a, s, (int)g);
#pragma unroll
            for (int e = 0; e < 4; ++e) a.cameras_out[g * 4 + e] = (cf && e < 2) ? (float)c[e] : a.cameras[g * 4 + e];
        }
    }
}

// ------------------------------------------------------------------ the launch list of both entry points: `rounds` filters, rounds + 1 stages of `iterations`
// PCG (lg_bundle_adjust_pcg): the solve is setup and `budget` times tracks, images, step instead of reduce, the Cholesky panels and the back substitution
template <int LOSS, bool ROBUST, bool FOCAL = false, bool PCG = false>
static int ba_enqueue(const std::conditional_t<PCG, BaPcgArgs, BaArgsOf<FOCAL>>& a, const BaLayout& L, int iterations, int rounds, hipStream_t s) {
    static_assert(!(PCG && FOCAL), "the iterative solver knows six unknowns per image");
    auto blocks = [](long long items) { return dim3((unsigned)((items + BA_THREADS - 1) / BA_THREADS)); };
    const dim3 th(BA_THREADS);
    const BaArgs& b = a;                                        // what the kernels that know no focal column take
    const int K = a.images, T = a.tracks;
    const long long all = std::max<long long>(std::max<long long>(L.nodes, T), K);
    hipLaunchKernelGGL(ba_init_kernel<FOCAL>, blocks(std::max<long long>(K, T)), th, 0, s, a);
    if (L.nodes) hipLaunchKernelGGL(ba_count_kernel<false>, blocks(L.nodes), th, 0, s, b);
    if (T) hipLaunchKernelGGL(ba_scan_kernel, dim3(1), dim3(BA_SCAN_THREADS), 0, s, b);
    if (L.nodes) hipLaunchKernelGGL(ba_fill_kernel, blocks(L.nodes), th, 0, s, b);
    if (T) hipLaunchKernelGGL(ba_sort_kernel, blocks(T), th, 0, s, b);
    hipLaunchKernelGGL((ba_cost_kernel<LOSS, FOCAL>), dim3(K), th, 0, s, a, 0);
    hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(64), 0, s, b, 1);
    for (int stage = 0; stage <= rounds; ++stage) {
        if (stage) {                                            // the filter and the rebuild of the lists from the nodes still in state 1
            hipLaunchKernelGGL(ba_filter_kernel<FOCAL>, blocks(all), th, 0, s, a, stage == 1 ? 1 : 0);
            if (L.nodes) hipLaunchKernelGGL(ba_count_kernel<true>, blocks(L.nodes), th, 0, s, b);
            if (T) hipLaunchKernelGGL(ba_scan_kernel, dim3(1), dim3(BA_SCAN_THREADS), 0, s, b);
            if (L.nodes) hipLaunchKernelGGL(ba_fill_kernel, blocks(L.nodes), th, 0, s, b);
            if (T) hipLaunchKernelGGL(ba_sort_kernel, blocks(T), th, 0, s, b);
            hipLaunchKernelGGL((ba_cost_kernel<LOSS, FOCAL>), dim3(K), th, 0, s, a, 0);
            hipLaunchKernelGGL(ba_restage_kernel, dim3(1), dim3(64), 0, s, b);
        }
        for (int it = 0; it < iterations; ++it) {
            if (T) hipLaunchKernelGGL((ba_points_kernel<LOSS, FOCAL>), blocks(T), th, 0, s, a);
            if constexpr (PCG) {
                const int lm = stage * iterations + it;
                hipLaunchKernelGGL(ba_pcg_setup_kernel<LOSS>, dim3(K), dim3(PCG_THREADS), 0, s, a, lm);
                for (int cg = 0; cg < a.budget; ++cg) {
                    if (T) hipLaunchKernelGGL(ba_pcg_tracks_kernel<LOSS>, blocks(T), th, 0, s, a, lm);
                    hipLaunchKernelGGL(ba_pcg_images_kernel<LOSS>, dim3(K), dim3(PCG_THREADS), 0, s, a, lm);
                    hipLaunchKernelGGL(ba_pcg_step_kernel, dim3(1), dim3(PCG_STEP_THREADS), 0, s, a, lm, cg);
                }
            } else {
                hipLaunchKernelGGL((ba_reduce_kernel<LOSS, FOCAL>), dim3(K, (K + BA_CHUNK<FOCAL> - 1) / BA_CHUNK<FOCAL>), th, 0, s, a);
                for_cholesky_panels((int)L.dim, 1, [&](int p, int tiles_below) {
                    hipLaunchKernelGGL(ba_cholesky_diag_kernel, dim3(1), th, 0, s, b, p);
                    hipLaunchKernelGGL(ba_cholesky_rows_kernel, dim3(tiles_below), th, 0, s, b, p);
                });
                hipLaunchKernelGGL(ba_backsolve_kernel<FOCAL>, dim3(1), th, 0, s, a);
            }
            if (T) hipLaunchKernelGGL((ba_trial_points_kernel<LOSS, FOCAL>), blocks(T), th, 0, s, a);
            hipLaunchKernelGGL((ba_cost_kernel<LOSS, FOCAL>), dim3(K), th, 0, s, a, 1);
            hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(64), 0, s, b, 0);
        }
    }
    hipLaunchKernelGGL((ba_scatter_kernel<ROBUST, FOCAL>), blocks(all), th, 0, s, a);
    if constexpr (PCG) hipLaunchKernelGGL(ba_pcg_summary_kernel, dim3(1), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

// the kernels' view of a checked call: the caller's arrays and the workspace carved by L
static BaArgs ba_args(const lg_bundle_io& io, const BaLayout& L) {
    const Carved ws(io.workspace);
    BaArgs a{};
    a.n = io.n; a.images = io.images; a.nodes = (int)L.nodes; a.tracks = io.tracks; a.dim = (int)L.dim;
    a.lambda0 = io.initial_damping; a.ftol = io.function_tolerance;
    a.kpts = io.kpts; a.num = io.num; a.track_id = reinterpret_cast<const long long*>(io.track_id); a.xyz = io.xyz; a.cameras = io.cameras; a.poses = io.poses;
    a.constant = io.constant_pose;
    a.head = ws.as<BaHead>(L.head); a.rec = ws.as<BaImage>(L.rec);
    a.pose = ws.f64(L.pose); a.delta = ws.f64(L.delta); a.icost = ws.f64(L.icost); a.S = ws.f64(L.S);
    a.list = ws.ints(L.list); a.limg = ws.ints(L.limg); a.tcnt = ws.ints(L.tcnt); a.toff = ws.ints(L.toff); a.tcur = ws.ints(L.tcur);
    a.X = ws.f64(L.X); a.Vinv = ws.f64(L.Vinv); a.y = ws.f64(L.y);
    a.poses_out = io.poses_out; a.xyz_out = io.xyz_out; a.points3d = io.points3d; a.node_state = io.node_state; a.obs_err = io.observation_error;
    a.summary = io.summary; a.status = io.status;
    return a;
}

// lg_bundle_adjust_robust and lg_bundle_adjust_focal: the robust settings behind a checked call's arguments, and the launch list with r's loss compiled in
template <bool FOCAL> static int ba_enqueue_robust(BaArgsOf<FOCAL> a, const BaRobustLayout& L, const lg_bundle_robust_io& r, void* hip_stream) {
    a.lc = r.loss_scale; a.lc2 = r.loss_scale * r.loss_scale; a.fe2 = r.max_reproj_error * r.max_reproj_error;
    a.tmov = r.filter_rounds > 0 ? Carved(r.base.workspace).ints(L.tmov) : nullptr;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    switch (r.loss) {
        case LG_BA_LOSS_HUBER: return ba_enqueue<LG_BA_LOSS_HUBER, true, FOCAL>(a, L.base, r.base.num_iterations, r.filter_rounds, s);
        case LG_BA_LOSS_CAUCHY: return ba_enqueue<LG_BA_LOSS_CAUCHY, true, FOCAL>(a, L.base, r.base.num_iterations, r.filter_rounds, s);
        default: return ba_enqueue<LG_BA_LOSS_SQUARED, true, FOCAL>(a, L.base, r.base.num_iterations, r.filter_rounds, s);
    }
}

// lg_bundle_adjust_pcg: the robust settings and the solver's arrays behind a checked call's arguments, and the launch list with the loss compiled in
static int ba_enqueue_pcg(const lg_bundle_pcg_io& io, const BaPcgLayout& L, void* hip_stream) {
    const lg_bundle_robust_io& r = io.base;
    const Carved ws(r.base.workspace);
    BaPcgArgs a{};
    static_cast<BaArgs&>(a) = ba_args(r.base, L.base.base);
    a.lc = r.loss_scale; a.lc2 = r.loss_scale * r.loss_scale; a.fe2 = r.max_reproj_error * r.max_reproj_error;
    a.tmov = r.filter_rounds > 0 ? ws.ints(L.base.tmov) : nullptr;
    a.ph = ws.as<BaPcgHead>(L.head); a.r = ws.f64(L.r); a.z = ws.f64(L.z); a.p = ws.f64(L.p); a.q = ws.f64(L.q); a.U = ws.f64(L.U); a.M = ws.f64(L.M);
    a.pq = ws.f64(L.pq); a.rz = ws.f64(L.rz); a.u = ws.f64(L.u);
    a.tol = io.cg_tolerance; a.budget = io.max_cg_iterations;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    switch (r.loss) {
        case LG_BA_LOSS_HUBER: return ba_enqueue<LG_BA_LOSS_HUBER, true, false, true>(a, L.base.base, r.base.num_iterations, r.filter_rounds, s);
        case LG_BA_LOSS_CAUCHY: return ba_enqueue<LG_BA_LOSS_CAUCHY, true, false, true>(a, L.base.base, r.base.num_iterations, r.filter_rounds, s);
        default: return ba_enqueue<LG_BA_LOSS_SQUARED, true, false, true>(a, L.base.base, r.base.num_iterations, r.filter_rounds, s);
    }
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_bundle_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags) {
    BaLayout L;
    return ba_layout(images, n, tracks, flags, L) ? -1 : L.total;
}

int lg_bundle_adjust(const lg_bundle_io* io, void* hip_stream) {
    if (!io) return set_error(LG_ERR_INVALID, "lg_bundle_adjust: null io");
    BaLayout L;
    if (const char* why = ba_layout(io->images, io->n, io->tracks, io->flags, L)) return set_error(LG_ERR_INVALID, std::string("lg_bundle_adjust: ") + why);
    if (const int rc = ba_check_settings("lg_bundle_adjust", "lg_bundle_workspace_bytes", *io, L.nodes, L.total)) return rc;
    return ba_enqueue<LG_BA_LOSS_SQUARED, false>(ba_args(*io, L), L, io->num_iterations, 0, static_cast<hipStream_t>(hip_stream));
}

int64_t lg_bundle_robust_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags) {
    BaRobustLayout L;
    return ba_robust_layout(images, n, tracks, flags, L) ? -1 : L.total;
}

int lg_bundle_adjust_robust(const lg_bundle_robust_io* io, void* hip_stream) {
    static const char* const stage = "lg_bundle_adjust_robust";
    if (!io) return set_error(LG_ERR_INVALID, std::string(stage) + ": null io");
    BaRobustLayout L;
    if (const char* why = ba_robust_layout(io->base.images, io->base.n, io->base.tracks, io->base.flags, L)) return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why);
    if (const char* why = ba_robust_settings_error(io->loss, io->loss_scale, io->filter_rounds, io->max_reproj_error))
        return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why);
    if (const int rc = ba_check_settings(stage, "lg_bundle_robust_workspace_bytes", io->base, L.base.nodes, L.total)) return rc;
    return ba_enqueue_robust<false>(ba_args(io->base, L.base), L, *io, hip_stream);
}

int64_t lg_bundle_focal_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags) {
    BaFocalLayout L;
    return ba_focal_layout(images, n, tracks, flags, L) ? -1 : L.total;
}

int lg_bundle_adjust_focal(const lg_bundle_focal_io* io, void* hip_stream) {
    static const char* const stage = "lg_bundle_adjust_focal";
    if (!io) return set_error(LG_ERR_INVALID, std::string(stage) + ": null io");
    const lg_bundle_robust_io& r = io->base;
    BaFocalLayout L;
    if (const char* why = ba_focal_layout(r.base.images, r.base.n, r.base.tracks, r.base.flags, L)) return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why);
    if (const int rc = ba_focal_check_settings(stage, *io, L)) return rc;
    const BaFocalArgs a{ba_args(r.base, L.base.base), io->constant_camera, Carved(r.base.workspace).f64(L.cam), io->cameras_out};
    return ba_enqueue_robust<true>(a, L.base, r, hip_stream);
}

int64_t lg_bundle_pcg_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags) {
    BaPcgLayout L;
    return ba_pcg_layout(images, n, tracks, flags, L) ? -1 : L.total;
}

int lg_bundle_adjust_pcg(const lg_bundle_pcg_io* io, void* hip_stream) {
    static const char* const stage = "lg_bundle_adjust_pcg";
    const auto refuse = [](const char* why) { return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why); };
    if (!io) return refuse("null io");
    const lg_bundle_robust_io& r = io->base;
    BaPcgLayout L;
    if (const char* why = ba_pcg_layout(r.base.images, r.base.n, r.base.tracks, r.base.flags, L)) return refuse(why);
    if (const char* why = ba_robust_settings_error(r.loss, r.loss_scale, r.filter_rounds, r.max_reproj_error)) return refuse(why);
    if (const char* why = ba_pcg_settings_error(r.base.num_iterations, r.filter_rounds, io->max_cg_iterations, io->pad, io->cg_tolerance)) return refuse(why);
    if (const int rc = ba_check_settings(stage, "lg_bundle_pcg_workspace_bytes", r.base, L.base.base.nodes, L.total)) return rc;
    return ba_enqueue_pcg(*io, L, hip_stream);
}

}  // extern "C"
