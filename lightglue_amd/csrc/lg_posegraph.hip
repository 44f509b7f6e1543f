// lightglue_amd — global poses from relative poses (lg_posegraph_solve; the definition is in include/lightglue_amd.h).  Launches per call:
//   pg_clear      one lane per image: counters, levels; the record of the call;
//   pg_classify   one lane per pair: its state (0, 1, 2), the usable pairs of every image counted by integer atomicAdd;
//   pg_scan       ONE workgroup: the offsets of the images' adjacency lists;
//   pg_fill       one lane per pair: a place in both lists by atomicAdd on the cursor (arrival order is arbitrary);
//   pg_sort       one lane per image: its list put into ascending (neighbour, pair) order by a heap sort (what the atomics left is gone);
//   pg_tree       ONE workgroup, one lane per image: the level-synchronous breadth-first tree, the initial rotations, state 3;
//   per rotation iteration: pg_rot_assemble (one workgroup per image row), pg_chol_diag + pg_chol_rows once per panel, pg_rot_update (ONE workgroup);
//   pg_select     ONE workgroup: rotation errors and state 4, directions, the baseline, the images that get a position, state 5;
//   per position iteration: pg_pos_assemble (one workgroup per image: its three rows), the two Cholesky launches per panel, pg_pos_update (ONE workgroup);
//   pg_output     one lane per image and pair.
// That is 8 + n (4 + 2 ceil(K / 48) + 2 ceil(3 K / 48)) launches for n iterations over K images: 104 at K = 16, n = 12; 584 at K = 256.  No kernel waits on
// another workgroup; every kernel of a stage returns at once when the stage's `done` is set in the record (uniform over the grid: only the update kernels
// write it).  No floating-point atomics: every sum runs over the image's sorted list.  Small matrices are indexed statically.  exp of a rotation vector and the
// position stage's ray steps (ray_block, ray_apply, ray_angle, ray_weight) are lg_solver_steps.h's, shared with lg_bundle.hip and lg_positioning.hip.
// lg_posegraph_solve_pcg runs the same list with both solves swapped and the two single-workgroup graph kernels widened: pg_tree_wide and pg_select_wide (ONE
// workgroup of 1 024 threads, images strided over the lanes), and per iteration of a stage pg_pcg_pairs (one lane per pair), pg_pcg_setup (one wave per
// image) and, budget times, pg_pcg_operator (one wave per image: q = A p, its p.q) and pg_pcg_step (ONE workgroup); last pg_pcg_summary.
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

constexpr int PG_THREADS = 256;
constexpr double PG_DEG = 180.0 / 3.14159265358979323846, PG_FLOOR = 1e-10;
static_assert(PG_THREADS == CH_THREADS && LG_BA_MAX_IMAGES <= PG_THREADS && LG_BA_CHOLESKY_BLOCK == CH_NB, "one lane per image; the Cholesky's workgroup");

struct PgHead { int done[2], iters[2], fail, pos_bad, baseline, base_pair; double cbase[3]; };
static_assert(sizeof(PgHead) <= 256, "the record of the call is 256 bytes");

struct PgArgs {
    int K, P, n, origin, baseline_in, min_inliers;
    double sigma, tau, max_rot;                             // radians, radians, degrees
    const long long* pairs; const float* R; const float* t; const float* w; const int* inl;
    PgHead* head; double* rot; double* cen; int* level; int* present; int* acount; int* aoff; int* acur; int* pstate; double* perr; double* dir;
    unsigned long long* adj; double* S;
    float* poses; unsigned char* image_state; unsigned char* pair_state; float* rot_err; float* dir_err; double* summary;
};

__device__ __forceinline__ int key_nbr(unsigned long long k) { return (int)(k >> 32); }
__device__ __forceinline__ int key_pair(unsigned long long k) { return (int)(k & 0xFFFFFFFFull); }

// C = A B, C = A^T B (3 x 3 row-major), each entry (x0 y0 + x1 y1) + x2 y2
__device__ __forceinline__ void mul33(const double* A, const double* B, double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mulT33(const double* A, const double* B, double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void widen9(const float* src, double (&M)[9]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] = (double)src[e];
}
// the log map of the definition
__device__ __forceinline__ void so3_log(const double (&M)[9], double (&om)[3]) {
    const double v[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
    const double tr = (M[0] + M[4]) + M[8];
    const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    double scale;
    if (nv < 1e-6) scale = tr < 0.0 ? 0.0 : 0.5;
    else scale = atan2(0.5 * nv, 0.5 * (tr - 1.0)) / nv;
#pragma unroll
    for (int e = 0; e < 3; ++e) om[e] = v[e] * scale;
}
// omega of pair p at the current rotations: log(R_b^T R_ab R_a)
__device__ __forceinline__ void pair_omega(const PgArgs& a, int p, int ia, int ib, double (&om)[3]) {
    double Rab[9], T[9], M[9];
    widen9(a.R + (long long)p * 9, Rab);
    mul33(Rab, a.rot + (long long)ia * 9, T);
    mulT33(a.rot + (long long)ib * 9, T, M);
    so3_log(M, om);
}

// ------------------------------------------------------------------ records, states 1 and 2, the adjacency
__global__ __launch_bounds__(PG_THREADS) void pg_clear_kernel(PgArgs a) {
    const int g = blockIdx.x * PG_THREADS + threadIdx.x;
    if (g == 0) { PgHead h{}; h.baseline = -1; h.base_pair = -1; *a.head = h; }
    if (g < a.K) { a.acount[g] = 0; a.acur[g] = 0; a.level[g] = -1; a.present[g] = 0; }
}

__global__ __launch_bounds__(PG_THREADS) void pg_classify_kernel(PgArgs a) {
    const int p = blockIdx.x * PG_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const long long ia = a.pairs[2 * (long long)p], ib = a.pairs[2 * (long long)p + 1];
    int state = 0;
    if (ia < 0 || ia >= a.K || ib < 0 || ib >= a.K || ia == ib) state = 1;
    else {
        double R[9];
        widen9(a.R + (long long)p * 9, R);
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 9; ++e) ok = ok && isfinite(R[e]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double s = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
                ok = ok && fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-3;
            }
        const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        const double t0 = (double)a.t[3 * (long long)p], t1 = (double)a.t[3 * (long long)p + 1], t2 = (double)a.t[3 * (long long)p + 2];
        const double tt = (t0 * t0 + t1 * t1) + t2 * t2, w = (double)a.w[p];
        ok = ok && det > 0.0 && isfinite(tt) && tt > 0.0 && isfinite(w) && w > 0.0;
        if (a.inl && a.inl[p] < a.min_inliers) ok = false;
        if (!ok) state = 2;
    }
    a.pstate[p] = state;
    if (state == 0) { atomicAdd(a.acount + ia, 1); atomicAdd(a.acount + ib, 1); }
}

__global__ __launch_bounds__(PG_THREADS) void pg_scan_kernel(PgArgs a) {
    if (threadIdx.x) return;
    int at = 0;                                             // at most 2 P <= 2^21
    for (int k = 0; k < a.K; ++k) { a.aoff[k] = at; at += a.acount[k]; }
    a.aoff[a.K] = at;
}

__global__ __launch_bounds__(PG_THREADS) void pg_fill_kernel(PgArgs a) {
    const int p = blockIdx.x * PG_THREADS + threadIdx.x;
    if (p >= a.P || a.pstate[p] != 0) return;
    const int ia = (int)a.pairs[2 * (long long)p], ib = (int)a.pairs[2 * (long long)p + 1];      // both in [0, K)
    const int qa = atomicAdd(a.acur + ia, 1), qb = atomicAdd(a.acur + ib, 1);
    if (qa < a.acount[ia]) a.adj[a.aoff[ia] + qa] = ((unsigned long long)ib << 32) | (unsigned)p;          // always: acount entries carry this image
    if (qb < a.acount[ib]) a.adj[a.aoff[ib] + qb] = ((unsigned long long)ia << 32) | (unsigned)p;
}

// one lane per image: heap sort of its keys (neighbour, pair), all distinct: the result does not depend on the order the atomics left
__global__ __launch_bounds__(PG_THREADS) void pg_sort_kernel(PgArgs a) {
    const int k = blockIdx.x * PG_THREADS + threadIdx.x;
    if (k >= a.K) return;
    unsigned long long* v = a.adj + a.aoff[k];
    const int len = a.acount[k];
    auto sift = [&](int root, int end) {
        const unsigned long long x = v[root];
        for (;;) {
            int child = 2 * root + 1;
            if (child >= end) break;
            if (child + 1 < end && v[child + 1] > v[child]) ++child;
            if (v[child] <= x) break;
            v[root] = v[child];
            root = child;
        }
        v[root] = x;
    };
    for (int r = len / 2 - 1; r >= 0; --r) sift(r, len);
    for (int end = len - 1; end > 0; --end) {
        const unsigned long long top = v[0];
        v[0] = v[end]; v[end] = top;
        sift(0, end);
    }
}

// ------------------------------------------------------------------ the tree: ONE workgroup, lane i = image i
__global__ __launch_bounds__(PG_THREADS) void pg_tree_kernel(PgArgs a) {
    __shared__ int lvl[PG_THREADS];
    const int i = threadIdx.x;
    const bool mine = i < a.K;
    lvl[i] = (mine && i == a.origin) ? 0 : -1;
    if (mine) {
#pragma unroll
        for (int e = 0; e < 9; ++e) a.rot[(long long)i * 9 + e] = (e % 4 == 0) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int L = 0; L < a.K; ++L) {
        int bj = -1, bp = -1;
        double bw = 0.0;
        if (mine && lvl[i] < 0) {
            const int beg = a.aoff[i], end = a.aoff[i + 1];
            for (int e = beg; e < end; ++e) {               // ascending (neighbour, pair): the first of the heaviest wins
                const unsigned long long key = a.adj[e];
                const int j = key_nbr(key), p = key_pair(key);
                const double w = (double)a.w[p];
                if (lvl[j] == L && (bp < 0 || w > bw)) { bj = j; bp = p; bw = w; }
            }
        }
        if (!__syncthreads_or(bp >= 0)) break;              // (a barrier: every lane has read lvl)
        if (bp >= 0) {
            double Rab[9], out[9];
            widen9(a.R + (long long)bp * 9, Rab);
            if ((int)a.pairs[2 * (long long)bp + 1] == i) mul33(Rab, a.rot + (long long)bj * 9, out);      // image i is b: R_ab R_a
            else mulT33(Rab, a.rot + (long long)bj * 9, out);                                               // image i is a: R_ab^T R_b
#pragma unroll
            for (int e = 0; e < 9; ++e) a.rot[(long long)i * 9 + e] = out[e];
            lvl[i] = L + 1;                                 // no lane reads lvl between the barrier above and the one below
        }
        __syncthreads();
    }
    if (mine) a.level[i] = lvl[i];
    for (int p = i; p < a.P; p += PG_THREADS)
        if (a.pstate[p] == 0 && lvl[(int)a.pairs[2 * (long long)p]] < 0) a.pstate[p] = 3;
}

// ------------------------------------------------------------------ rotation averaging: row i of the weighted Laplacian and of the three right-hand sides
__global__ __launch_bounds__(PG_THREADS) void pg_rot_assemble_kernel(PgArgs a, double sigma_it) {
    __shared__ int sJ[PG_THREADS];
    __shared__ double sW[PG_THREADS], sOm[PG_THREADS][3];
    if (a.head->done[0]) return;
    const int i = blockIdx.x, t = threadIdx.x, K = a.K;
    double* row = a.S + (long long)i * K;
    for (int c = t; c < K; c += PG_THREADS) row[c] = 0.0;
    const bool free_i = a.level[i] >= 0 && i != a.origin;
    __syncthreads();
    if (!free_i) {
        if (t == 0) { row[i] = 1.0; for (int r = 0; r < 3; ++r) a.S[(long long)(K + r) * K + i] = 0.0; }
        return;
    }
    const int beg = a.aoff[i], end = a.aoff[i + 1];
    double diag = 0.0, rhs[3] = {0.0, 0.0, 0.0}, run = 0.0;
    int runj = -1;
    for (int e0 = beg; e0 < end; e0 += PG_THREADS) {
        __syncthreads();
        int j = -1;
        if (e0 + t < end) {
            const unsigned long long key = a.adj[e0 + t];
            const int p = key_pair(key);
            if (a.pstate[p] == 0) {
                const int ia = (int)a.pairs[2 * (long long)p], ib = (int)a.pairs[2 * (long long)p + 1];
                double om[3];
                pair_omega(a, p, ia, ib, om);
                const double th = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]), q = th / sigma_it;
                const double w = (double)a.w[p] / (1.0 + q * q), sg = ib == i ? 1.0 : -1.0;
                j = key_nbr(key);
                sW[t] = w;
#pragma unroll
                for (int r = 0; r < 3; ++r) sOm[t][r] = sg * (w * om[r]);
            }
        }
        sJ[t] = j;
        __syncthreads();
        if (t == 0) {
            const int m = min(PG_THREADS, end - e0);
            for (int q = 0; q < m; ++q) {
                const int jq = sJ[q];
                if (jq < 0) continue;
                diag += sW[q];
                rhs[0] += sOm[q][0]; rhs[1] += sOm[q][1]; rhs[2] += sOm[q][2];
                if (jq < i && a.level[jq] >= 0 && jq != a.origin) {      // the lower triangle; a fixed image's column drops out
                    if (jq != runj) { if (runj >= 0) row[runj] = run; runj = jq; run = 0.0; }
                    run -= sW[q];
                }
            }
        }
    }
    if (t == 0) {
        if (runj >= 0) row[runj] = run;
        row[i] = diag;
        for (int r = 0; r < 3; ++r) a.S[(long long)(K + r) * K + i] = rhs[r];
    }
}

__global__ __launch_bounds__(CH_THREADS) void pg_chol_diag_kernel(PgArgs a, int stage, int dim, int panel) {
    __shared__ CholeskyDiagLds m;
    if (a.head->done[stage]) return;
    cholesky_diag(a.S, dim, panel, PG_FLOOR, &a.head->fail, m);
}
__global__ __launch_bounds__(CH_THREADS) void pg_chol_rows_kernel(PgArgs a, int stage, int dim, int nrhs, int panel) {
    __shared__ CholeskyRowsLds m;
    if (a.head->done[stage]) return;
    cholesky_rows(a.S, dim, nrhs, panel, panel + blockIdx.x, m);
}

// ONE workgroup: the three steps, R_i <- R_i exp(delta_i), convergence
__global__ __launch_bounds__(PG_THREADS) void pg_rot_update_kernel(PgArgs a, int it, int final_scale) {
    __shared__ double sd[3 * LG_BA_MAX_IMAGES], red[PG_THREADS];
    __shared__ CholeskySolveLds m;
    if (a.head->done[0]) return;
    const int i = threadIdx.x, K = a.K;
    cholesky_backsolve(a.S, K, 3, sd, m);
    double mx = 0.0;
    int bad = 0;
    if (i < K) {
        const double x[3] = {sd[i], sd[K + i], sd[2 * K + i]};
        if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) bad = 1;
        mx = fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2]));
        if (a.level[i] >= 0 && i != a.origin) {
            double* Ri = a.rot + (long long)i * 9;
            double Q[9], out[9];
            so3_exp(x, Q);
            mul33(Ri, Q, out);
#pragma unroll
            for (int e = 0; e < 9; ++e) Ri[e] = out[e];
        }
    }
    red[i] = mx;
    bad = __syncthreads_or(bad);
    if (i == 0) {
        for (int q = 1; q < PG_THREADS; ++q) mx = fmax(mx, red[q]);
        a.head->iters[0] = it + 1;
        a.head->fail = 0;
        if (final_scale && !bad && mx < 1e-10) a.head->done[0] = 1;
    }
}

// ------------------------------------------------------------------ between the stages: ONE workgroup
__global__ __launch_bounds__(PG_THREADS) void pg_select_kernel(PgArgs a) {
    __shared__ int cur[PG_THREADS], sBase[2];
    const int i = threadIdx.x, K = a.K;
    for (int p = i; p < a.P; p += PG_THREADS) {
        double err = __builtin_nan("");
        if (a.pstate[p] == 0) {
            const int ia = (int)a.pairs[2 * (long long)p], ib = (int)a.pairs[2 * (long long)p + 1];
            double om[3];
            pair_omega(a, p, ia, ib, om);
            err = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]) * PG_DEG;
            if (err > a.max_rot) a.pstate[p] = 4;
            else {
                const double t0 = (double)a.t[3 * (long long)p], t1 = (double)a.t[3 * (long long)p + 1], t2 = (double)a.t[3 * (long long)p + 2];
                const double nt = sqrt((t0 * t0 + t1 * t1) + t2 * t2), u[3] = {t0 / nt, t1 / nt, t2 / nt};
                const double* Rb = a.rot + (long long)ib * 9;
#pragma unroll
                for (int r = 0; r < 3; ++r) a.dir[3 * (long long)p + r] = -((Rb[r] * u[0] + Rb[3 + r] * u[1]) + Rb[6 + r] * u[2]);
            }
        }
        a.perr[p] = err;
    }
    __syncthreads();
    if (i == 0) {                                           // the baseline: the origin's heaviest usable pair (to baseline_in if one is given)
        int bj = -1, bp = -1;
        double bw = 0.0;
        for (int e = a.aoff[a.origin]; e < a.aoff[a.origin + 1]; ++e) {
            const unsigned long long key = a.adj[e];
            const int j = key_nbr(key), p = key_pair(key);
            const double w = (double)a.w[p];
            if (a.pstate[p] == 0 && (a.baseline_in < 0 || j == a.baseline_in) && (bp < 0 || w > bw)) { bj = j; bp = p; bw = w; }
        }
        sBase[0] = bj; sBase[1] = bp;
    }
    __syncthreads();
    const int base = sBase[0], bp = sBase[1];
    const bool mine = i < K;
    if (base < 0) {                                         // no pair fixes the scale: no positions
        if (mine) { a.present[i] = 0; for (int r = 0; r < 3; ++r) a.cen[3 * i + r] = 0.0; }
        if (i == 0) { a.head->done[1] = 1; a.head->pos_bad = 1; }
        return;
    }
    cur[i] = mine && a.level[i] >= 0;
    __syncthreads();
    for (int round = 0; round < K; ++round) {
        int nxt = cur[i];
        if (mine && cur[i] && i != a.origin && i != base) {
            int count = 0, last = -1;
            for (int e = a.aoff[i]; e < a.aoff[i + 1]; ++e) {
                const unsigned long long key = a.adj[e];
                const int j = key_nbr(key);
                if (j != last && a.pstate[key_pair(key)] == 0 && cur[j]) { ++count; last = j; }
            }
            nxt = count >= 2;
        }
        const int changed = __syncthreads_or(nxt != cur[i]);
        cur[i] = nxt;
        __syncthreads();
        if (!changed) break;
    }
    if (mine) {
        a.present[i] = cur[i];
        const double sg = (int)a.pairs[2 * (long long)bp] == a.origin ? 1.0 : -1.0;
        for (int r = 0; r < 3; ++r) a.cen[3 * i + r] = i == base ? sg * a.dir[3 * (long long)bp + r] : 0.0;
    }
    if (i == 0) {
        a.head->baseline = base; a.head->base_pair = bp;
        const double sg = (int)a.pairs[2 * (long long)bp] == a.origin ? 1.0 : -1.0;
        for (int r = 0; r < 3; ++r) a.head->cbase[r] = sg * a.dir[3 * (long long)bp + r];
    }
    for (int p = i; p < a.P; p += PG_THREADS)
        if (a.pstate[p] == 0 && !(cur[(int)a.pairs[2 * (long long)p]] && cur[(int)a.pairs[2 * (long long)p + 1]])) a.pstate[p] = 5;
}

// ------------------------------------------------------------------ position averaging: the three rows of image i
__global__ __launch_bounds__(PG_THREADS) void pg_pos_assemble_kernel(PgArgs a, int it, double tau_it) {
    __shared__ int sJ[PG_THREADS];
    __shared__ double sM[PG_THREADS][6];
    if (a.head->done[1]) return;
    const int i = blockIdx.x, t = threadIdx.x, dim = 3 * a.K, base = a.head->baseline;
    double* rows = a.S + (long long)3 * i * dim;
    double* z = a.S + (long long)dim * dim;
    for (int c = t; c < 3 * dim; c += PG_THREADS) rows[c] = 0.0;
    const bool free_i = a.present[i] && i != a.origin && i != base;
    __syncthreads();
    if (!free_i) {
        if (t < 3) { rows[(long long)t * dim + 3 * i + t] = 1.0; z[3 * i + t] = 0.0; }
        return;
    }
    const int beg = a.aoff[i], end = a.aoff[i + 1];
    const double cb[3] = {a.head->cbase[0], a.head->cbase[1], a.head->cbase[2]};
    double diag[6] = {0, 0, 0, 0, 0, 0}, run[6] = {0, 0, 0, 0, 0, 0}, rhs[3] = {0, 0, 0};
    int runj = -1;
    // the symmetric block (xx, xy, xz, yy, yz, zz) -> rows [3 i, 3 i + 3) x columns [3 j, 3 j + 3)
    auto flush = [&](int j, const double (&B)[6]) {
        double* o = rows + 3 * j;
        o[0] = B[0]; o[1] = B[1]; o[2] = B[2];
        o[dim] = B[1]; o[dim + 1] = B[3]; o[dim + 2] = B[4];
        o[2 * dim] = B[2]; o[2 * dim + 1] = B[4]; o[2 * dim + 2] = B[5];
    };
    for (int e0 = beg; e0 < end; e0 += PG_THREADS) {
        __syncthreads();
        int j = -1;
        if (e0 + t < end) {
            const unsigned long long key = a.adj[e0 + t];
            const int p = key_pair(key);
            if (a.pstate[p] == 0) {
                const int ia = (int)a.pairs[2 * (long long)p], ib = (int)a.pairs[2 * (long long)p + 1];
                const double* d = a.dir + 3 * (long long)p;
                double rho = 1.0;
                if (it > 0) {
                    const double e[3] = {a.cen[3 * ib] - a.cen[3 * ia], a.cen[3 * ib + 1] - a.cen[3 * ia + 1], a.cen[3 * ib + 2] - a.cen[3 * ia + 2]};
                    rho = ray_weight(d, e, tau_it);
                }
                j = key_nbr(key);
                ray_block(d, (double)a.w[p] * rho, sM[t]);
            }
        }
        sJ[t] = j;
        __syncthreads();
        if (t == 0) {
            const int m = min(PG_THREADS, end - e0);
            for (int q = 0; q < m; ++q) {
                const int jq = sJ[q];
                if (jq < 0) continue;
                const double (&M)[6] = sM[q];
#pragma unroll
                for (int s = 0; s < 6; ++s) diag[s] += M[s];
                if (jq == base) {                           // the baseline's known centre moves to the right-hand side
                    double y[3];
                    ray_apply(M, cb, y);
                    rhs[0] += y[0]; rhs[1] += y[1]; rhs[2] += y[2];
                } else if (jq < i && jq != a.origin) {      // a free image (state 0: it is present), the lower block triangle
                    if (jq != runj) {
                        if (runj >= 0) flush(runj, run);
                        runj = jq;
#pragma unroll
                        for (int s = 0; s < 6; ++s) run[s] = 0.0;
                    }
#pragma unroll
                    for (int s = 0; s < 6; ++s) run[s] -= M[s];
                }
            }
        }
    }
    if (t == 0) {
        if (runj >= 0) flush(runj, run);
        flush(i, diag);
        for (int r = 0; r < 3; ++r) z[3 * i + r] = rhs[r];
    }
}

// ONE workgroup: the centres, convergence, a failed pivot
__global__ __launch_bounds__(PG_THREADS) void pg_pos_update_kernel(PgArgs a, int it, int final_scale) {
    __shared__ double sd[3 * LG_BA_MAX_IMAGES], red[PG_THREADS];
    __shared__ CholeskySolveLds m;
    if (a.head->done[1]) return;
    const int i = threadIdx.x, K = a.K, base = a.head->baseline;
    cholesky_backsolve(a.S, 3 * K, 1, sd, m);
    double mx = 0.0;
    int bad = 0;
    if (i < K && a.present[i] && i != a.origin && i != base) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double x = sd[3 * i + r], step = fabs(x - a.cen[3 * i + r]);
            if (!isfinite(step)) bad = 1;
            mx = fmax(mx, step);
            a.cen[3 * i + r] = x;
        }
    }
    red[i] = mx;
    bad = __syncthreads_or(bad);
    if (i == 0) {
        for (int q = 1; q < PG_THREADS; ++q) mx = fmax(mx, red[q]);
        a.head->iters[1] = it + 1;
        if (a.head->fail) a.head->pos_bad = 1;
        a.head->fail = 0;
        if (final_scale && !bad && mx < 1e-12) a.head->done[1] = 1;
    }
}

// ------------------------------------------------------------------ the outputs
__global__ __launch_bounds__(PG_THREADS) void pg_output_kernel(PgArgs a) {
    const int g = blockIdx.x * PG_THREADS + threadIdx.x;
    const PgHead h = *a.head;
    const bool positions = !h.pos_bad;
    const float nanf_ = __builtin_nanf("");
    if (g == 0) {
        int posed = 0;
        for (int k = 0; k < a.K; ++k) posed += positions && a.present[k];
        a.summary[0] = (double)a.origin; a.summary[1] = (double)h.baseline; a.summary[2] = (double)posed; a.summary[3] = (double)h.iters[0];
        a.summary[4] = (double)h.iters[1]; a.summary[5] = positions ? 1.0 : 0.0; a.summary[6] = 0.0; a.summary[7] = 0.0;
    }
    if (g < a.K) {
        const bool in = a.level[g] >= 0, posed = positions && a.present[g];
        const double* R = a.rot + (long long)g * 9;
        const double* c = a.cen + (long long)g * 3;
        float* o = a.poses + (long long)g * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int e = 0; e < 3; ++e) o[4 * r + e] = in ? (float)R[3 * r + e] : nanf_;
            o[4 * r + 3] = posed ? (float)minus_Rc(R, c, r) : nanf_;
        }
        a.image_state[g] = (unsigned char)(posed ? 0 : in ? 1 : 2);
    }
    if (g < a.P) {
        const int st = a.pstate[g];
        float de = nanf_;
        if (st == 0 && positions) {
            const int ia = (int)a.pairs[2 * (long long)g], ib = (int)a.pairs[2 * (long long)g + 1];
            const double e[3] = {a.cen[3 * ib] - a.cen[3 * ia], a.cen[3 * ib + 1] - a.cen[3 * ia + 1], a.cen[3 * ib + 2] - a.cen[3 * ia + 2]};
            de = (float)(ray_angle(a.dir + 3 * (long long)g, e) * PG_DEG);
        }
        a.pair_state[g] = (unsigned char)st;
        a.rot_err[g] = (float)a.perr[g];
        a.dir_err[g] = de;
    }
}

// ------------------------------------------------------------------ lg_posegraph_solve_pcg: both stages solved by preconditioned conjugate gradients
// Neither system is formed: q = A p is one pass over every image's list.  Every launch of both budgets is enqueued; the step kernel alone writes PgPcgHead
// (the tree clears it), and once `done` names the running iteration of the running stage, or the stage has ended, the rest return at once.  The tree and
// the selection stand here a second time with the images strided over 1 024 lanes: the old entry point's kernels keep their text and instruction streams
// (profiles/global_poses_pcg.md).  Every list sum is lane-strided partials and THE fold of list_sum below; the image dots are image_sum (lg_solver_steps.h)
constexpr int PGW_THREADS = 1024, PGW_PER = LG_BA_PCG_MAX_IMAGES / PGW_THREADS, PGC_WAVE = 64;
static_assert(PGW_PER * PGW_THREADS == LG_BA_PCG_MAX_IMAGES, "the wide kernels hold PGW_PER images per lane");

struct PgPcgHead { double rz, rz0; int done, block_bad, cg[2], onbudget[2], failures, pad; };        // done: 1 + (stage x n + iteration) whose solve ended
static_assert(sizeof(PgPcgHead) <= 256, "the record of the solver is 256 bytes");
struct PgPcgArgs : PgArgs {
    PgPcgHead* ph; double* pm; double* r; double* z; double* p; double* q; double* x; double* D; double* Di; double* pq; double* rz;   // pm [pairs][6]; D [images][6]; Di [images][9]
    double tol; int budget[2];
};

// THE fold of a list sum: partial l += partial l + h for l < h, h = 32 .. 1; lane 0 holds the result
__device__ __forceinline__ double list_sum(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_down(v, h, 64);
    return v;
}
__device__ __forceinline__ double dot3(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
template <int STAGE> __device__ __forceinline__ bool pg_free(const PgPcgArgs& a, int i) {
    if (STAGE == 0) return a.level[i] >= 0 && i != a.origin;
    return a.present[i] && i != a.origin && i != a.head->baseline;
}
template <int STAGE> __device__ __forceinline__ bool pg_pcg_idle(const PgPcgArgs& a, int it) { return a.head->done[STAGE] || a.ph->done == 1 + STAGE * a.n + it; }

// the tree of pg_tree_kernel, lane t = images t, t + 1024, ..; the record of the solver
__global__ __launch_bounds__(PGW_THREADS) void pg_tree_wide_kernel(PgPcgArgs a) {
    __shared__ int lvl[LG_BA_PCG_MAX_IMAGES];
    const int t = threadIdx.x;
    if (t == 0) *a.ph = PgPcgHead{};
    for (int i = t; i < a.K; i += PGW_THREADS) {
        lvl[i] = i == a.origin ? 0 : -1;
#pragma unroll
        for (int e = 0; e < 9; ++e) a.rot[(long long)i * 9 + e] = (e % 4 == 0) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int L = 0; L < a.K; ++L) {
        int bj[PGW_PER], bp[PGW_PER], any = 0;
#pragma unroll
        for (int s = 0; s < PGW_PER; ++s) {
            const int i = t + s * PGW_THREADS;
            bj[s] = -1; bp[s] = -1;
            double bw = 0.0;
            if (i < a.K && lvl[i] < 0) {
                const int beg = a.aoff[i], end = a.aoff[i + 1];
                for (int e = beg; e < end; ++e) {           // ascending (neighbour, pair): the first of the heaviest wins
                    const unsigned long long key = a.adj[e];
                    const int j = key_nbr(key), p = key_pair(key);
                    const double w = (double)a.w[p];
                    if (lvl[j] == L && (bp[s] < 0 || w > bw)) { bj[s] = j; bp[s] = p; bw = w; }
                }
            }
            any |= bp[s] >= 0;
        }
        if (!__syncthreads_or(any)) break;                  // (a barrier: every lane has read lvl)
#pragma unroll
        for (int s = 0; s < PGW_PER; ++s) {
            if (bp[s] < 0) continue;
            const int i = t + s * PGW_THREADS;
            double Rab[9], out[9];
            widen9(a.R + (long long)bp[s] * 9, Rab);
            if ((int)a.pairs[2 * (long long)bp[s] + 1] == i) mul33(Rab, a.rot + (long long)bj[s] * 9, out);
            else mulT33(Rab, a.rot + (long long)bj[s] * 9, out);
#pragma unroll
            for (int e = 0; e < 9; ++e) a.rot[(long long)i * 9 + e] = out[e];
            lvl[i] = L + 1;                                 // no lane reads lvl between the barrier above and the one below
        }
        __syncthreads();
    }
    for (int i = t; i < a.K; i += PGW_THREADS) a.level[i] = lvl[i];
    for (int p = t; p < a.P; p += PGW_THREADS)
        if (a.pstate[p] == 0 && lvl[(int)a.pairs[2 * (long long)p]] < 0) a.pstate[p] = 3;
}

// the selection of pg_select_kernel, lane t = images t, t + 1024, ..
__global__ __launch_bounds__(PGW_THREADS) void pg_select_wide_kernel(PgPcgArgs a) {
    __shared__ int cur[LG_BA_PCG_MAX_IMAGES], sBase[2];
    const int t = threadIdx.x, K = a.K;
    for (int p = t; p < a.P; p += PGW_THREADS) {
        double err = __builtin_nan("");
        if (a.pstate[p] == 0) {
            const int ia = (int)a.pairs[2 * (long long)p], ib = (int)a.pairs[2 * (long long)p + 1];
            double om[3];
            pair_omega(a, p, ia, ib, om);
            err = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]) * PG_DEG;
            if (err > a.max_rot) a.pstate[p] = 4;
            else {
                const double t0 = (double)a.t[3 * (long long)p], t1 = (double)a.t[3 * (long long)p + 1], t2 = (double)a.t[3 * (long long)p + 2];
                const double nt = sqrt((t0 * t0 + t1 * t1) + t2 * t2), u[3] = {t0 / nt, t1 / nt, t2 / nt};
                const double* Rb = a.rot + (long long)ib * 9;
#pragma unroll
                for (int r = 0; r < 3; ++r) a.dir[3 * (long long)p + r] = -((Rb[r] * u[0] + Rb[3 + r] * u[1]) + Rb[6 + r] * u[2]);
            }
        }
        a.perr[p] = err;
    }
    __syncthreads();
    if (t == 0) {                                           // the baseline: the origin's heaviest usable pair (to baseline_in if one is given)
        int bj = -1, bp = -1;
        double bw = 0.0;
        for (int e = a.aoff[a.origin]; e < a.aoff[a.origin + 1]; ++e) {
            const unsigned long long key = a.adj[e];
            const int j = key_nbr(key), p = key_pair(key);
            const double w = (double)a.w[p];
            if (a.pstate[p] == 0 && (a.baseline_in < 0 || j == a.baseline_in) && (bp < 0 || w > bw)) { bj = j; bp = p; bw = w; }
        }
        sBase[0] = bj; sBase[1] = bp;
    }
    __syncthreads();
    const int base = sBase[0], bp = sBase[1];
    if (base < 0) {                                         // no pair fixes the scale: no positions
        for (int i = t; i < K; i += PGW_THREADS) { a.present[i] = 0; for (int r = 0; r < 3; ++r) a.cen[3 * i + r] = 0.0; }
        if (t == 0) { a.head->done[1] = 1; a.head->pos_bad = 1; }
        return;
    }
    for (int i = t; i < K; i += PGW_THREADS) cur[i] = a.level[i] >= 0;
    __syncthreads();
    for (int round = 0; round < K; ++round) {
        int nxt[PGW_PER], moved = 0;
#pragma unroll
        for (int s = 0; s < PGW_PER; ++s) {
            const int i = t + s * PGW_THREADS;
            nxt[s] = i < K ? cur[i] : 0;
            if (i < K && cur[i] && i != a.origin && i != base) {
                int count = 0, last = -1;
                for (int e = a.aoff[i]; e < a.aoff[i + 1]; ++e) {
                    const unsigned long long key = a.adj[e];
                    const int j = key_nbr(key);
                    if (j != last && a.pstate[key_pair(key)] == 0 && cur[j]) { ++count; last = j; }
                }
                nxt[s] = count >= 2;
                moved |= nxt[s] != cur[i];
            }
        }
        const int changed = __syncthreads_or(moved);
#pragma unroll
        for (int s = 0; s < PGW_PER; ++s)
            if (t + s * PGW_THREADS < K) cur[t + s * PGW_THREADS] = nxt[s];
        __syncthreads();
        if (!changed) break;
    }
    const double sg = (int)a.pairs[2 * (long long)bp] == a.origin ? 1.0 : -1.0;
    for (int i = t; i < K; i += PGW_THREADS) {
        a.present[i] = cur[i];
        for (int r = 0; r < 3; ++r) a.cen[3 * i + r] = i == base ? sg * a.dir[3 * (long long)bp + r] : 0.0;
    }
    if (t == 0) {
        a.head->baseline = base; a.head->base_pair = bp;
        for (int r = 0; r < 3; ++r) a.head->cbase[r] = sg * a.dir[3 * (long long)bp + r];
    }
    for (int p = t; p < a.P; p += PGW_THREADS)
        if (a.pstate[p] == 0 && !(cur[(int)a.pairs[2 * (long long)p]] && cur[(int)a.pairs[2 * (long long)p + 1]])) a.pstate[p] = 5;
}

// one lane per pair of state 0: (w', w' omega) at the current rotations, or the six entries of M at the current centres
template <int STAGE> __global__ __launch_bounds__(PG_THREADS) void pg_pcg_pairs_kernel(PgPcgArgs a, int it, double scale_it) {
    if (a.head->done[STAGE]) return;
    const int p = blockIdx.x * PG_THREADS + threadIdx.x;
    if (p >= a.P || a.pstate[p] != 0) return;
    const int ia = (int)a.pairs[2 * (long long)p], ib = (int)a.pairs[2 * (long long)p + 1];
    double* m = a.pm + 6 * (long long)p;
    if (STAGE == 0) {
        double om[3];
        pair_omega(a, p, ia, ib, om);
        const double th = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]), q = th / scale_it;
        const double w = (double)a.w[p] / (1.0 + q * q);
        m[0] = w; m[1] = w * om[0]; m[2] = w * om[1]; m[3] = w * om[2];
    } else {
        const double* d = a.dir + 3 * (long long)p;
        double rho = 1.0, M[6];
        if (it > 0) {
            const double e[3] = {a.cen[3 * ib] - a.cen[3 * ia], a.cen[3 * ib + 1] - a.cen[3 * ia + 1], a.cen[3 * ib + 2] - a.cen[3 * ia + 2]};
            rho = ray_weight(d, e, scale_it);
        }
        ray_block(d, (double)a.w[p] * rho, M);
#pragma unroll
        for (int s = 0; s < 6; ++s) m[s] = M[s];
    }
}

// one wave per image: D, D^-1, b, the warm-started r, z = D^-1 r, p = z, x0 and the image's partial of r.z.  Lane l takes the entries l, l + 64, ..
template <int STAGE> __global__ __launch_bounds__(PGC_WAVE) void pg_pcg_setup_kernel(PgPcgArgs a) {
    if (a.head->done[STAGE]) return;
    const int i = blockIdx.x, l = threadIdx.x;
    const long long at = 3 * (long long)i;
    if (!pg_free<STAGE>(a, i)) {
        if (l < 3) { a.r[at + l] = 0.0; a.z[at + l] = 0.0; a.p[at + l] = 0.0; a.q[at + l] = 0.0; a.x[at + l] = 0.0; }
        if (l == 0) { a.pq[i] = 0.0; a.rz[i] = 0.0; }
        return;
    }
    const int beg = a.aoff[i], end = a.aoff[i + 1], base = a.head->baseline;
    const double cb[3] = {a.head->cbase[0], a.head->cbase[1], a.head->cbase[2]};
    double d[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, tx[3] = {0, 0, 0};
    for (int e = beg + l; e < end; e += PGC_WAVE) {
        const unsigned long long key = a.adj[e];
        const int p = key_pair(key);
        if (a.pstate[p] != 0) continue;
        const double* m = a.pm + 6 * (long long)p;
        if (STAGE == 0) {
            const double sg = (int)a.pairs[2 * (long long)p + 1] == i ? 1.0 : -1.0;
            d[0] += m[0];
            b[0] += sg * m[1]; b[1] += sg * m[2]; b[2] += sg * m[3];
        } else {
            const double M[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
            const int j = key_nbr(key);
            double y[3];
#pragma unroll
            for (int s = 0; s < 6; ++s) d[s] += M[s];
            if (j == base) { ray_apply(M, cb, y); b[0] += y[0]; b[1] += y[1]; b[2] += y[2]; }
            else { ray_apply(M, a.cen + 3 * (long long)j, y); tx[0] += y[0]; tx[1] += y[1]; tx[2] += y[2]; }
        }
    }
#pragma unroll
    for (int s = 0; s < (STAGE == 0 ? 1 : 6); ++s) d[s] = list_sum(d[s]);
#pragma unroll
    for (int s = 0; s < 3; ++s) { b[s] = list_sum(b[s]); if (STAGE == 1) tx[s] = list_sum(tx[s]); }
    if (l != 0) return;
    double r[3], z[3], x0[3] = {0.0, 0.0, 0.0}, Di[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (STAGE == 0) {
        Di[0][0] = 1.0 / d[0];
#pragma unroll
        for (int s = 0; s < 3; ++s) { r[s] = b[s]; z[s] = Di[0][0] * r[s]; }
    } else {
        double ax[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) x0[s] = a.cen[at + s];
        ray_apply(d, x0, ax);
#pragma unroll
        for (int s = 0; s < 3; ++s) r[s] = b[s] - (ax[s] - tx[s]);
        if (!tri_inverse3(d, Di)) atomicOr(&a.ph->block_bad, 1);
#pragma unroll
        for (int s = 0; s < 3; ++s) z[s] = (Di[s][0] * r[0] + Di[s][1] * r[1]) + Di[s][2] * r[2];
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) a.D[6 * (long long)i + s] = d[s];
#pragma unroll
    for (int s = 0; s < 9; ++s) a.Di[9 * (long long)i + s] = Di[s / 3][s % 3];
#pragma unroll
    for (int s = 0; s < 3; ++s) { a.r[at + s] = r[s]; a.z[at + s] = z[s]; a.p[at + s] = z[s]; a.q[at + s] = 0.0; a.x[at + s] = x0[s]; }
    a.rz[i] = dot3(r, z); a.pq[i] = 0.0;
}

// one wave per image: q_i = D_i p_i - the list sum of w' p_j (of M p_j), and the image's partial of p.q.  The p of an image that is not free is 0
template <int STAGE> __global__ __launch_bounds__(PGC_WAVE) void pg_pcg_operator_kernel(PgPcgArgs a, int it) {
    if (pg_pcg_idle<STAGE>(a, it)) return;                  // uniform over the grid: no launch between the step kernels writes either
    const int i = blockIdx.x, l = threadIdx.x;
    if (!pg_free<STAGE>(a, i)) return;                      // q and the partial stay 0 (pg_pcg_setup_kernel)
    const int beg = a.aoff[i], end = a.aoff[i + 1];
    double acc[3] = {0, 0, 0};
    for (int e = beg + l; e < end; e += PGC_WAVE) {
        const unsigned long long key = a.adj[e];
        const int p = key_pair(key);
        if (a.pstate[p] != 0) continue;
        const double* m = a.pm + 6 * (long long)p;
        const double* pj = a.p + 3 * (long long)key_nbr(key);
        if (STAGE == 0) { const double w = m[0]; acc[0] += w * pj[0]; acc[1] += w * pj[1]; acc[2] += w * pj[2]; }
        else {
            const double M[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
            double y[3];
            ray_apply(M, pj, y);
            acc[0] += y[0]; acc[1] += y[1]; acc[2] += y[2];
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) acc[s] = list_sum(acc[s]);
    if (l != 0) return;
    const double pi[3] = {a.p[3 * (long long)i], a.p[3 * (long long)i + 1], a.p[3 * (long long)i + 2]};
    double q[3];
    if (STAGE == 0) {
        const double D = a.D[6 * (long long)i];
#pragma unroll
        for (int s = 0; s < 3; ++s) q[s] = D * pi[s] - acc[s];
    } else {
        double D[6], y[3];
#pragma unroll
        for (int s = 0; s < 6; ++s) D[s] = a.D[6 * (long long)i + s];
        ray_apply(D, pi, y);
#pragma unroll
        for (int s = 0; s < 3; ++s) q[s] = y[s] - acc[s];
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) a.q[3 * (long long)i + s] = q[s];
    a.pq[i] = dot3(pi, q);
}

// ONE workgroup, solver iteration `cg` of iteration `it` of a stage: p.q, alpha, x, r, z = D^-1 r, r.z, the stopping test, beta, p; the record; when the
// solve ends the stage's update (pg_rot_update_kernel's, pg_pos_update_kernel's).  Strided loops over the images
template <int STAGE> __global__ __launch_bounds__(PGW_THREADS) void pg_pcg_step_kernel(PgPcgArgs a, int it, int cg, int final_scale) {
    __shared__ double part[IMAGE_SUM_PARTIALS];
    const int t = threadIdx.x, K = a.K;
    PgPcgHead& h = *a.ph;
    if (pg_pcg_idle<STAGE>(a, it)) return;
    double rz = h.rz, rz0 = h.rz0;                          // (read by all before lane 0 writes them again, behind the barriers of image_sum)
    bool end = false, bad = false;
    if (cg == 0) {
        rz = rz0 = image_sum(a.rz, K, part);
        if (t == 0) { h.rz = rz; h.rz0 = rz0; }
        if ((STAGE == 1 && h.block_bad) || !(isfinite(rz) && rz >= 0.0)) bad = true;
        else if (rz == 0.0) end = true;                     // the residual is 0 (no free image among them): x = x0
    }
    double rz_new = rz;
    if (!bad && !end) {
        const double pq = image_sum(a.pq, K, part);
        if (!(isfinite(pq) && pq > 0.0)) bad = true;
        else {
            const double alpha = rz / pq;
            for (int k = t; k < K; k += PGW_THREADS) {
                if (!pg_free<STAGE>(a, k)) continue;
                const long long at = 3 * (long long)k;
                const double* Di = a.Di + 9 * (long long)k;
                double r[3], z[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    a.x[at + e] = a.x[at + e] + alpha * a.p[at + e];
                    r[e] = a.r[at + e] - alpha * a.q[at + e];
                    a.r[at + e] = r[e];
                }
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    z[e] = STAGE == 0 ? Di[0] * r[e] : (Di[3 * e] * r[0] + Di[3 * e + 1] * r[1]) + Di[3 * e + 2] * r[2];
                    a.z[at + e] = z[e];
                }
                a.rz[k] = dot3(r, z);
            }
            rz_new = image_sum(a.rz, K, part);
            if (t == 0) h.cg[STAGE] += 1;
            if (!(isfinite(rz_new) && rz_new >= 0.0)) bad = true;
            else {
                const bool reached = sqrt(rz_new) <= a.tol * sqrt(rz0);
                end = reached || cg == a.budget[STAGE] - 1;
                if (end && !reached && t == 0) h.onbudget[STAGE] += 1;
            }
        }
    }
    if (bad && t == 0) h.failures += 1;
    if (bad && STAGE == 1) {                                // a failed block or recurrence: no positions, the stage ends with the centres it has
        if (t == 0) { a.head->pos_bad = 1; a.head->iters[1] = it + 1; a.head->done[1] = 1; }
        return;
    }
    if (!bad && !end) {
        const double beta = rz_new / rz;
        for (int k = t; k < K; k += PGW_THREADS) {
            if (!pg_free<STAGE>(a, k)) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e) a.p[3 * (long long)k + e] = a.z[3 * (long long)k + e] + beta * a.p[3 * (long long)k + e];
        }
        if (t == 0) h.rz = rz_new;
        return;
    }
    if (t == 0) h.done = 1 + STAGE * a.n + it;
    double mx = 0.0;
    int wrong = 0;
    for (int k = t; k < K; k += PGW_THREADS) {
        if (!pg_free<STAGE>(a, k)) continue;
        const double x[3] = {a.x[3 * (long long)k], a.x[3 * (long long)k + 1], a.x[3 * (long long)k + 2]};
        if (STAGE == 0) {
            if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) wrong = 1;
            mx = fmax(mx, fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2])));
            double* Ri = a.rot + (long long)k * 9;
            double Q[9], out[9];
            so3_exp(x, Q);
            mul33(Ri, Q, out);
#pragma unroll
            for (int e = 0; e < 9; ++e) Ri[e] = out[e];
        } else {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const double step = fabs(x[e] - a.cen[3 * (long long)k + e]);
                if (!isfinite(step)) wrong = 1;
                mx = fmax(mx, step);
                a.cen[3 * (long long)k + e] = x[e];
            }
        }
    }
    __syncthreads();                                        // part has been read by all
    if (t < IMAGE_SUM_PARTIALS) part[t] = 0.0;
    __syncthreads();
    for (int s = 0; s < PGW_THREADS / IMAGE_SUM_PARTIALS; ++s) {       // the largest step: a maximum does not depend on the order
        if (t / IMAGE_SUM_PARTIALS == s) part[t % IMAGE_SUM_PARTIALS] = fmax(part[t % IMAGE_SUM_PARTIALS], mx);
        __syncthreads();
    }
    wrong = __syncthreads_or(wrong);
    if (t == 0) {
        for (int q = 1; q < IMAGE_SUM_PARTIALS; ++q) mx = fmax(mx, part[q]);
        mx = fmax(mx, part[0]);
        a.head->iters[STAGE] = it + 1;
        if (final_scale && !wrong && mx < (STAGE == 0 ? 1e-10 : 1e-12)) a.head->done[STAGE] = 1;
    }
}

// one lane, behind pg_output_kernel: the counters of the solver
__global__ void pg_pcg_summary_kernel(PgPcgArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    const PgPcgHead h = *a.ph;
    a.summary[6] = (double)h.failures; a.summary[8] = (double)h.cg[0]; a.summary[9] = (double)h.cg[1];
    a.summary[10] = (double)h.onbudget[0]; a.summary[11] = (double)h.onbudget[1];
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_posegraph_workspace_bytes(int64_t images, int64_t pairs, uint32_t flags) {
    PgLayout L;
    return pg_layout(images, pairs, flags, L) ? -1 : L.total;
}

int lg_posegraph_solve(const lg_posegraph_io* io, void* hip_stream) {
    if (!io) return set_error(LG_ERR_INVALID, "lg_posegraph_solve: null io");
    PgLayout L;
    if (const char* why = pg_layout(io->images, io->pairs, io->flags, L)) return set_error(LG_ERR_INVALID, std::string("lg_posegraph_solve: ") + why);
    if (const char* why = pg_settings_error(io->images, io->num_iterations, io->origin, io->baseline, io->rotation_scale, io->max_rotation_error,
                                            io->direction_scale))
        return set_error(LG_ERR_INVALID, std::string("lg_posegraph_solve: ") + why);
    if (!io->pair_index || !io->rotations || !io->translations || !io->weights || !io->poses || !io->image_state || !io->pair_state || !io->rotation_error ||
        !io->direction_error || !io->summary)
        return set_error(LG_ERR_INVALID, "lg_posegraph_solve: null pointer among pair_index, rotations, translations, weights, poses, image_state, pair_state, "
                                         "rotation_error, direction_error, summary");
    if (const int rc = check_workspace("lg_posegraph_solve", "lg_posegraph_workspace_bytes", io->workspace, io->workspace_bytes, L.total)) return rc;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Carved ws(io->workspace);
    const double rad = 3.14159265358979323846 / 180.0;
    PgArgs a{};
    a.K = io->images; a.P = io->pairs; a.n = io->num_iterations; a.origin = io->origin; a.baseline_in = io->baseline; a.min_inliers = io->min_inliers;
    a.sigma = io->rotation_scale * rad; a.tau = io->direction_scale * rad; a.max_rot = io->max_rotation_error;
    a.pairs = reinterpret_cast<const long long*>(io->pair_index); a.R = io->rotations; a.t = io->translations; a.w = io->weights; a.inl = io->num_inliers;
    a.head = ws.as<PgHead>(L.head); a.rot = ws.f64(L.rot); a.cen = ws.f64(L.cen);
    a.level = ws.ints(L.level); a.present = ws.ints(L.present); a.acount = ws.ints(L.acount); a.aoff = ws.ints(L.aoff); a.acur = ws.ints(L.acur);
    a.pstate = ws.ints(L.pstate); a.perr = ws.f64(L.perr); a.dir = ws.f64(L.dir); a.adj = ws.as<unsigned long long>(L.adj); a.S = ws.f64(L.S);
    a.poses = io->poses; a.image_state = io->image_state; a.pair_state = io->pair_state; a.rot_err = io->rotation_error; a.dir_err = io->direction_error;
    a.summary = io->summary;

    auto blocks = [](long long items) { return dim3((unsigned)((items + PG_THREADS - 1) / PG_THREADS)); };
    const dim3 th(PG_THREADS);
    const int K = io->images, P = io->pairs, n = io->num_iterations;
    auto factor = [&](int stage, int dim, int nrhs) {
        for_cholesky_panels(dim, nrhs, [&](int p, int tiles_below) {
            hipLaunchKernelGGL(pg_chol_diag_kernel, dim3(1), th, 0, s, a, stage, dim, p);
            hipLaunchKernelGGL(pg_chol_rows_kernel, dim3(tiles_below), th, 0, s, a, stage, dim, nrhs, p);
        });
    };
    hipLaunchKernelGGL(pg_clear_kernel, blocks(K), th, 0, s, a);
    hipLaunchKernelGGL(pg_classify_kernel, blocks(P), th, 0, s, a);
    hipLaunchKernelGGL(pg_scan_kernel, dim3(1), th, 0, s, a);
    hipLaunchKernelGGL(pg_fill_kernel, blocks(P), th, 0, s, a);
    hipLaunchKernelGGL(pg_sort_kernel, blocks(K), th, 0, s, a);
    hipLaunchKernelGGL(pg_tree_kernel, dim3(1), th, 0, s, a);
    for (int it = 0; it < n; ++it) {
        const int halvings = std::max(0, n - 5 - it);
        hipLaunchKernelGGL(pg_rot_assemble_kernel, dim3(K), th, 0, s, a, a.sigma * std::ldexp(1.0, halvings));
        factor(0, K, 3);
        hipLaunchKernelGGL(pg_rot_update_kernel, dim3(1), th, 0, s, a, it, halvings == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL(pg_select_kernel, dim3(1), th, 0, s, a);
    for (int it = 0; it < n; ++it) {
        const int halvings = std::max(0, n - 6 - it);
        hipLaunchKernelGGL(pg_pos_assemble_kernel, dim3(K), th, 0, s, a, it, a.tau * std::ldexp(1.0, halvings));
        factor(1, 3 * K, 1);
        hipLaunchKernelGGL(pg_pos_update_kernel, dim3(1), th, 0, s, a, it, halvings == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL(pg_output_kernel, blocks(std::max(K, P)), th, 0, s, a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

int64_t lg_posegraph_pcg_workspace_bytes(int64_t images, int64_t pairs, uint32_t flags) {
    PgPcgLayout L;
    return pg_pcg_layout(images, pairs, flags, L) ? -1 : L.total;
}

int lg_posegraph_solve_pcg(const lg_posegraph_pcg_io* pio, void* hip_stream) {
    static const char* const stage = "lg_posegraph_solve_pcg";
    const auto refuse = [](const char* why) { return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why); };
    if (!pio) return refuse("null io");
    const lg_posegraph_io* io = &pio->base;
    PgPcgLayout L;
    if (const char* why = pg_pcg_layout(io->images, io->pairs, io->flags, L)) return refuse(why);
    if (const char* why = pg_settings_error(io->images, io->num_iterations, io->origin, io->baseline, io->rotation_scale, io->max_rotation_error,
                                            io->direction_scale))
        return refuse(why);
    if (const char* why = pg_pcg_settings_error(io->num_iterations, pio->rotation_cg_iterations, pio->position_cg_iterations, pio->cg_tolerance)) return refuse(why);
    if (!io->pair_index || !io->rotations || !io->translations || !io->weights || !io->poses || !io->image_state || !io->pair_state || !io->rotation_error ||
        !io->direction_error || !io->summary)
        return refuse("null pointer among pair_index, rotations, translations, weights, poses, image_state, pair_state, rotation_error, direction_error, summary");
    if (const int rc = check_workspace(stage, "lg_posegraph_pcg_workspace_bytes", io->workspace, io->workspace_bytes, L.total)) return rc;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const Carved ws(io->workspace);
    const PgLayout& B = L.base;
    const double rad = 3.14159265358979323846 / 180.0;
    PgPcgArgs a{};
    a.K = io->images; a.P = io->pairs; a.n = io->num_iterations; a.origin = io->origin; a.baseline_in = io->baseline; a.min_inliers = io->min_inliers;
    a.sigma = io->rotation_scale * rad; a.tau = io->direction_scale * rad; a.max_rot = io->max_rotation_error;
    a.pairs = reinterpret_cast<const long long*>(io->pair_index); a.R = io->rotations; a.t = io->translations; a.w = io->weights; a.inl = io->num_inliers;
    a.head = ws.as<PgHead>(B.head); a.rot = ws.f64(B.rot); a.cen = ws.f64(B.cen);
    a.level = ws.ints(B.level); a.present = ws.ints(B.present); a.acount = ws.ints(B.acount); a.aoff = ws.ints(B.aoff); a.acur = ws.ints(B.acur);
    a.pstate = ws.ints(B.pstate); a.perr = ws.f64(B.perr); a.dir = ws.f64(B.dir); a.adj = ws.as<unsigned long long>(B.adj); a.S = nullptr;
    a.poses = io->poses; a.image_state = io->image_state; a.pair_state = io->pair_state; a.rot_err = io->rotation_error; a.dir_err = io->direction_error;
    a.summary = io->summary;
    a.ph = ws.as<PgPcgHead>(L.head); a.pm = ws.f64(L.pm); a.r = ws.f64(L.r); a.z = ws.f64(L.z); a.p = ws.f64(L.p); a.q = ws.f64(L.q); a.x = ws.f64(L.x);
    a.D = ws.f64(L.D); a.Di = ws.f64(L.Di); a.pq = ws.f64(L.pq); a.rz = ws.f64(L.rz);
    a.tol = pio->cg_tolerance; a.budget[0] = pio->rotation_cg_iterations; a.budget[1] = pio->position_cg_iterations;
    const PgArgs& dense = a;                                // what the launches shared with lg_posegraph_solve read

    auto blocks = [](long long items) { return dim3((unsigned)((items + PG_THREADS - 1) / PG_THREADS)); };
    const dim3 th(PG_THREADS), wide(PGW_THREADS), wave(PGC_WAVE);
    const int K = io->images, P = io->pairs, n = io->num_iterations;
    hipLaunchKernelGGL(pg_clear_kernel, blocks(K), th, 0, s, dense);
    hipLaunchKernelGGL(pg_classify_kernel, blocks(P), th, 0, s, dense);
    hipLaunchKernelGGL(pg_scan_kernel, dim3(1), th, 0, s, dense);
    hipLaunchKernelGGL(pg_fill_kernel, blocks(P), th, 0, s, dense);
    hipLaunchKernelGGL(pg_sort_kernel, blocks(K), th, 0, s, dense);
    hipLaunchKernelGGL(pg_tree_wide_kernel, dim3(1), wide, 0, s, a);
    for (int it = 0; it < n; ++it) {
        const int halvings = std::max(0, n - 5 - it);
        hipLaunchKernelGGL(pg_pcg_pairs_kernel<0>, blocks(P), th, 0, s, a, it, a.sigma * std::ldexp(1.0, halvings));
        hipLaunchKernelGGL(pg_pcg_setup_kernel<0>, dim3(K), wave, 0, s, a);
        for (int cg = 0; cg < a.budget[0]; ++cg) {
            hipLaunchKernelGGL(pg_pcg_operator_kernel<0>, dim3(K), wave, 0, s, a, it);
            hipLaunchKernelGGL(pg_pcg_step_kernel<0>, dim3(1), wide, 0, s, a, it, cg, halvings == 0 ? 1 : 0);
        }
    }
    hipLaunchKernelGGL(pg_select_wide_kernel, dim3(1), wide, 0, s, a);
    for (int it = 0; it < n; ++it) {
        const int halvings = std::max(0, n - 6 - it);
        hipLaunchKernelGGL(pg_pcg_pairs_kernel<1>, blocks(P), th, 0, s, a, it, a.tau * std::ldexp(1.0, halvings));
        hipLaunchKernelGGL(pg_pcg_setup_kernel<1>, dim3(K), wave, 0, s, a);
        for (int cg = 0; cg < a.budget[1]; ++cg) {
            hipLaunchKernelGGL(pg_pcg_operator_kernel<1>, dim3(K), wave, 0, s, a, it);
            hipLaunchKernelGGL(pg_pcg_step_kernel<1>, dim3(1), wide, 0, s, a, it, cg, halvings == 0 ? 1 : 0);
        }
    }
    hipLaunchKernelGGL(pg_output_kernel, blocks(std::max(K, P)), th, 0, s, dense);
    hipLaunchKernelGGL(pg_pcg_summary_kernel, dim3(1), wave, 0, s, a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

}  // extern "C"
