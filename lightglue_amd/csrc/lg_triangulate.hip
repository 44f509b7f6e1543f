// lightglue_amd — tracks and multi-view triangulation with known poses (lg_triangulate; the definition is in include/lightglue_amd.h).  Eight launches per call:
//   tri_init      one lane per node, pair and image: parent[v] = v, the counters cleared; the pair's status; the image's record in fp64 (R, t, c = -R^T t, camera, ok);
//   tri_union     one lane per row of matches0: the edge's two nodes are united by a lock-free union-find (below);
//   tri_flatten   one lane per node: root[v] = find(v) into an array of its own (parent is read-only here), the nodes of every root counted by integer atomicAdd;
//   tri_scan      ONE workgroup: an exclusive scan over the roots with >= 2 nodes gives every component its index (ascending root = ascending lowest node) and
//                 the offset of its list;
//   tri_fill      one lane per node: the node takes a place in its component's list by atomicAdd on the component's cursor.  Arrival order is arbitrary;
//   tri_tracks    one lane per component: a list no longer than max_track_length is put into ascending node order (insertion sort in place: what the atomics
//                 left is gone), conflicts are two adjacent entries of one image, then the geometry in fp64: the lane streams the observations and the cached image
//                 records and holds 6 + 3 accumulators and X in registers; every small matrix is indexed statically (no scratch: profiles/triangulate.md);
//   tri_number    ONE workgroup: an exclusive scan over the components' "state 1" flags gives the dense track ids; xyz, track_length, track_error, counts;
//   tri_scatter   one lane per node: points3d, track_id, node_state.
// The robust mode (lg_triangulate_robust) runs the first five as they are and then, in the place of the last three,
//   tri_robust          ONE WAVE per component: rank sort, the observations in the wave's LDS slice, up to max_tracks rounds of two-view hypotheses (lanes stride
//                       over them), an integer score, an integer wave maximum for the winner, the per-image consensus and tri_geometry on it by one lane;
//   tri_number_robust   ONE workgroup: the scan over the (component, round) slots; tri_scatter_robust: one lane per node.
// No kernel waits on another workgroup: the two scans are single workgroups, and the union loop retries only when its compare-and-swap lost to another lane's
// progress.  Everything behind tri_fill reads sorted lists and fixed orders, so every output is the same bits whatever the atomics' interleaving was.
#include <algorithm>
#include <cmath>
#include <string>

#include "lg_host_call.h"
#include "lg_kernels.h"
#include "lg_solve3.h"
#include "../../include/lightglue_amd.h"

#pragma clang fp contract(off)

namespace lg {

constexpr int TRI_THREADS = 256, TRI_SCAN_THREADS = 1024, TRI_GN_STEPS = 5;

struct TriImage { double R[9], t[3], c[3], cam[4]; int ok, pad; };                  // 160 bytes per image
static_assert(sizeof(TriImage) == 160, "lg_triangulate_workspace_bytes counts 160 bytes");
struct TriHead { int components, entries; };

struct TriArgs {
    int pairs, n, images, nodes, max_len, refine, tracks_only, angle_test;
    double max_err, cos_min;
    const float* kpts; const int* num; const int* index0; const int* index1; const long long* matches0; const float* cameras; const float* poses;
    TriHead* head; TriImage* rec; int* parent; int* root; int* cnt; int* off; int* comp; int* cursor; int* list;      // workspace, per node
    int* croot; int* cstate; int* tid; float* cres;                                                                   // workspace, per component
    float* points3d; long long* track_id; unsigned char* node_state; float* xyz; int* track_length; float* track_error; int* counts; int* status;
};

// the camera rule of one image: camera_ok (lg_common.h: the rule of every geometry entry point), and a finite pose
__device__ __forceinline__ bool tri_image_ok(const TriArgs& a, int k) {
    bool ok = camera_ok(a.cameras + (long long)k * 4);
    const float* p = a.poses + (long long)k * 12;
#pragma unroll
    for (int e = 0; e < 12; ++e) ok = ok && isfinite(p[e]);
    return ok;
}

// ------------------------------------------------------------------ 1. records, statuses, parent[v] = v
__global__ __launch_bounds__(TRI_THREADS) void tri_init_kernel(TriArgs a) {
    const long long g = (long long)blockIdx.x * TRI_THREADS + threadIdx.x;
    if (g == 0) *a.head = TriHead{0, 0};
    if (g < a.nodes) { a.parent[g] = (int)g; a.cnt[g] = 0; a.cursor[g] = 0; }
    if (g < a.images) {
        const int k = (int)g;
        TriImage im{};
        im.ok = 1;
        if (!a.tracks_only) {
            im.ok = tri_image_ok(a, k) ? 1 : 0;
            const float* p = a.poses + (long long)k * 12;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int j = 0; j < 3; ++j) im.R[3 * r + j] = (double)p[4 * r + j];
                im.t[r] = (double)p[4 * r + 3];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) im.c[j] = -((im.R[j] * im.t[0] + im.R[3 + j] * im.t[1]) + im.R[6 + j] * im.t[2]);
#pragma unroll
            for (int e = 0; e < 4; ++e) im.cam[e] = (double)a.cameras[(long long)k * 4 + e];
        }
        a.rec[k] = im;
    }
    if (g < a.pairs) {
        const int i0 = a.index0[g], i1 = a.index1[g];
        int st = LG_OK;
        if ((unsigned)i0 >= (unsigned)a.images || (unsigned)i1 >= (unsigned)a.images || i0 == i1) st = LG_ERR_INDEX;
        else if (!a.tracks_only && !(tri_image_ok(a, i0) && tri_image_ok(a, i1))) st = LG_ERR_CAMERA;
        a.status[g] = st;
    }
}

// ------------------------------------------------------------------ 2. union
__device__ __forceinline__ int tri_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// THE INVARIANT: parent[v] <= v at every instant (tri_init writes v; the only later writes are the compare-and-swap below, which puts lo < hi at hi, and the
// atomicMin here, which only lowers).  So a find is a strictly descending walk over non-negative integers: it ends after at most x steps whatever other lanes
// do meanwhile, and `p >= x` ends it even over memory that does not hold the invariant.  A node that has a parent below it never becomes a root again.
template <bool HALVE> __device__ __forceinline__ int tri_find(int* parent, int x) {
    for (;;) {
        const int p = tri_load(parent + x);
        if (p >= x || p < 0) return x;
        if (HALVE) {                                       // path halving: the grandparent is an ancestor of x below p
            const int gp = tri_load(parent + p);
            if (gp >= 0 && gp < p) atomicMin(parent + x, gp);
        }
        x = p;
    }
}

__global__ __launch_bounds__(TRI_THREADS) void tri_union_kernel(TriArgs a) {
    const long long e = (long long)blockIdx.x * TRI_THREADS + threadIdx.x;
    const int n = a.n;
    if (e >= (long long)a.pairs * n) return;
    const int pair = (int)(e / n), i = (int)(e % n);
    const int i0 = a.index0[pair], i1 = a.index1[pair];
    if ((unsigned)i0 >= (unsigned)a.images || (unsigned)i1 >= (unsigned)a.images || i0 == i1) return;
    if (!(a.rec[i0].ok && a.rec[i1].ok)) return;
    if (i >= live_rows(a.num, i0, n)) return;              // rows at or beyond num are unmatched and never read
    const long long m = a.matches0[e];
    if (m < 0 || m >= live_rows(a.num, i1, n)) return;     // live rows <= n
    int u = i0 * n + i, v = i1 * n + (int)m;               // both < images n = nodes
    // Lock-free: the higher root is hooked under the lower.  The loop comes round again only when the compare-and-swap found parent[hi] != hi, that is when
    // ANOTHER lane's hook of hi succeeded in between; every success takes one root away for good and there are at most `nodes` roots, so the retries of all
    // lanes together are bounded by the successes of all lanes together: no lane waits for another, none holds anything another needs.  A lane that lost goes
    // on from what the compare-and-swap returned, hi's parent below hi, so max(u, v) falls in every round: at most hi rounds even if every load were stale.
    for (;;) {
        u = tri_find<true>(a.parent, u); v = tri_find<true>(a.parent, v);
        if (u == v) break;
        const int hi = max(u, v), lo = min(u, v);
        const int old = atomicCAS(a.parent + hi, hi, lo);
        if (old == hi) break;
        if (old < 0 || old > hi) break;                    // not memory this call wrote: nothing to unite
        u = old; v = lo;
    }
}

// ------------------------------------------------------------------ 3. flatten and count
__global__ __launch_bounds__(TRI_THREADS) void tri_flatten_kernel(TriArgs a) {
    const int v = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (v >= a.nodes) return;
    const int r = tri_find<false>(a.parent, v);            // r <= v < nodes
    a.root[v] = r;
    atomicAdd(a.cnt + r, 1);
}

// ------------------------------------------------------------------ 4. / 7. the two scans: ONE workgroup, a contiguous share per thread, two passes
// exclusive scan of (x, y) per thread over the workgroup; the totals come back in tx, ty.  Inside a wave by shuffles, across the 16 waves through
// sh: __shared__ int[2 * TRI_SCAN_WAVES].  Integers: the order of the additions changes nothing.  Every thread calls
constexpr int TRI_SCAN_WAVES = TRI_SCAN_THREADS / 64;
__device__ __forceinline__ void tri_block_scan(int& x, int& y, int& tx, int& ty, int* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ix = x, iy = y;                                    // inclusive inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ux = __shfl_up(ix, o, 64), uy = __shfl_up(iy, o, 64);
        if (lane >= o) { ix += ux; iy += uy; }
    }
    __syncthreads();
    if (lane == 63) { sh[2 * wave] = ix; sh[2 * wave + 1] = iy; }
    __syncthreads();
    int bx = 0, by = 0;
    tx = 0; ty = 0;
    for (int w = 0; w < TRI_SCAN_WAVES; ++w) {
        const int vx = sh[2 * w], vy = sh[2 * w + 1];
        if (w < wave) { bx += vx; by += vy; }
        tx += vx; ty += vy;
    }
    x = bx + ix - x; y = by + iy - y;
}

__global__ __launch_bounds__(TRI_SCAN_THREADS) void tri_scan_kernel(TriArgs a) {
    __shared__ int sh[2 * TRI_SCAN_WAVES];
    const int share = (a.nodes + TRI_SCAN_THREADS - 1) / TRI_SCAN_THREADS;
    const int beg = min((int)threadIdx.x * share, a.nodes), end = min(beg + share, a.nodes);
    int comps = 0, entries = 0, tc, te;
    for (int v = beg; v < end; ++v) if (a.root[v] == v && a.cnt[v] >= 2) { ++comps; entries += a.cnt[v]; }
    tri_block_scan(comps, entries, tc, te, sh);
    for (int v = beg; v < end; ++v)
        if (a.root[v] == v && a.cnt[v] >= 2) {             // comps < nodes / 2 + 1 and entries + cnt[v] <= nodes: every node is counted once
            a.comp[v] = comps; a.off[v] = entries; a.croot[comps] = v;
            ++comps; entries += a.cnt[v];
        }
    if (threadIdx.x == 0) *a.head = TriHead{tc, te};
}

// ------------------------------------------------------------------ 5. fill
__global__ __launch_bounds__(TRI_THREADS) void tri_fill_kernel(TriArgs a) {
    const int v = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (v >= a.nodes) return;
    const int r = a.root[v], len = a.cnt[r];
    if (len < 2) return;
    const int at = atomicAdd(a.cursor + r, 1);
    if (at < len) a.list[a.off[r] + at] = v;               // always: cnt[r] nodes have this root
}

// ------------------------------------------------------------------ 6. one lane per component (the 3 x 3 elimination: lg_solve3.h)
struct TriProj { double px, py, pz; };
__device__ __forceinline__ TriProj tri_project(const TriImage& im, const double (&X)[3]) {
    return {((im.R[0] * X[0] + im.R[1] * X[1]) + im.R[2] * X[2]) + im.t[0], ((im.R[3] * X[0] + im.R[4] * X[1]) + im.R[5] * X[2]) + im.t[1],
            ((im.R[6] * X[0] + im.R[7] * X[1]) + im.R[8] * X[2]) + im.t[2]};
}

// one observation (x, y) of image `im` added to the sums of the linear start: S += I - d d^T, B += c - d (d . c)
__device__ __forceinline__ void tri_add_ray(const TriImage& im, float x, float y, double (&S)[6], double (&B)[3]) {
    const double xh = (double)((x - (float)im.cam[2]) / (float)im.cam[0]), yh = (double)((y - (float)im.cam[3]) / (float)im.cam[1]);
    double d[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) d[e] = (im.R[e] * xh + im.R[3 + e] * yh) + im.R[6 + e];
    const double nrm = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);          // of the rotated vector: a float32 R is orthonormal to 1e-7 only
#pragma unroll
    for (int e = 0; e < 3; ++e) d[e] = d[e] / nrm;
    const double dc = (d[0] * im.c[0] + d[1] * im.c[1]) + d[2] * im.c[2];
    S[0] += 1.0 - d[0] * d[0]; S[1] += -(d[0] * d[1]); S[2] += -(d[0] * d[2]);
    S[3] += 1.0 - d[1] * d[1]; S[4] += -(d[1] * d[2]); S[5] += 1.0 - d[2] * d[2];
#pragma unroll
    for (int e = 0; e < 3; ++e) B[e] += im.c[e] - d[e] * dc;
}

// false: pz <= 0 at X (err is not written); otherwise err: the reprojection error of the observation (x, y) of image `im`
__device__ __forceinline__ bool tri_obs_error(const TriImage& im, float x, float y, const double (&X)[3], double& err) {
    const TriProj p = tri_project(im, X);
    if (!(p.pz > 0.0)) return false;
    const double iz = 1.0 / p.pz;
    const double rx = ((im.cam[0] * p.px) * iz + im.cam[2]) - (double)x, ry = ((im.cam[1] * p.py) * iz + im.cam[3]) - (double)y;
    err = sqrt(rx * rx + ry * ry);
    return true;
}

// the state of one track (4 .. 7, or 1) and its point and mean error; lst: its observations in ascending node order
__device__ __forceinline__ int tri_geometry(const TriArgs& a, const int* lst, int len, double (&X)[3], double& mean_err) {
    const int n = a.n;
    double S[6] = {0, 0, 0, 0, 0, 0}, B[3] = {0, 0, 0};
    for (int j = 0; j < len; ++j) {
        const int v = lst[j];
        const float* kp = a.kpts + (long long)v * 2;
        tri_add_ray(a.rec[v / n], kp[0], kp[1], S, B);
    }
    if (!tri_solve3(S, B, X)) return 4;
    if (a.refine) {
        double Y[3] = {X[0], X[1], X[2]};
        bool kept = true;
        for (int step = 0; step < TRI_GN_STEPS && kept; ++step) {
            double H[6] = {0, 0, 0, 0, 0, 0}, G[3] = {0, 0, 0};
            for (int j = 0; j < len; ++j) {
                const int v = lst[j];
                const TriImage& im = a.rec[v / n];
                const TriProj p = tri_project(im, Y);
                if (!(p.pz > 0.0)) continue;
                const float* kp = a.kpts + (long long)v * 2;
                const double iz = 1.0 / p.pz, fx = im.cam[0], fy = im.cam[1];
                const double rx = ((fx * p.px) * iz + im.cam[2]) - (double)kp[0], ry = ((fy * p.py) * iz + im.cam[3]) - (double)kp[1];
                const double ax = fx * iz, az = -(((fx * p.px) * iz) * iz), by = fy * iz, bz = -(((fy * p.py) * iz) * iz);
                double J0[3], J1[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) { J0[e] = ax * im.R[e] + az * im.R[6 + e]; J1[e] = by * im.R[3 + e] + bz * im.R[6 + e]; }
                H[0] += J0[0] * J0[0] + J1[0] * J1[0]; H[1] += J0[0] * J0[1] + J1[0] * J1[1]; H[2] += J0[0] * J0[2] + J1[0] * J1[2];
                H[3] += J0[1] * J0[1] + J1[1] * J1[1]; H[4] += J0[1] * J0[2] + J1[1] * J1[2]; H[5] += J0[2] * J0[2] + J1[2] * J1[2];
#pragma unroll
                for (int e = 0; e < 3; ++e) G[e] += J0[e] * rx + J1[e] * ry;
            }
            const double ng[3] = {-G[0], -G[1], -G[2]};
            double s[3];
            kept = tri_solve3(H, ng, s);
#pragma unroll
            for (int e = 0; e < 3; ++e) Y[e] = Y[e] + s[e];
            kept = kept && isfinite(Y[0]) && isfinite(Y[1]) && isfinite(Y[2]);
        }
        if (kept) { X[0] = Y[0]; X[1] = Y[1]; X[2] = Y[2]; }
    }
    bool behind = false, far = false;
    double sum = 0.0;
    for (int j = 0; j < len; ++j) {
        const int v = lst[j];
        const float* kp = a.kpts + (long long)v * 2;
        double err;
        if (!tri_obs_error(a.rec[v / n], kp[0], kp[1], X, err)) { behind = true; continue; }
        far = far || !(err <= a.max_err);
        sum += err;
    }
    if (behind) return 5;
    if (far) return 6;
    mean_err = sum / (double)len;
    if (a.angle_test) {
        bool wide = false;
        for (int i = 0; i + 1 < len && !wide; ++i) {
            const TriImage& ii = a.rec[lst[i] / n];
            const double u[3] = {X[0] - ii.c[0], X[1] - ii.c[1], X[2] - ii.c[2]};
            const double nu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
            for (int j = i + 1; j < len && !wide; ++j) {
                const TriImage& ij = a.rec[lst[j] / n];
                const double w[3] = {X[0] - ij.c[0], X[1] - ij.c[1], X[2] - ij.c[2]};
                const double nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
                wide = (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2] <= (a.cos_min * nu) * nw;
            }
        }
        if (!wide) return 7;
    }
    return 1;
}

__global__ __launch_bounds__(TRI_THREADS) void tri_tracks_kernel(TriArgs a) {
    const int c = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (c >= a.head->components) return;                   // components <= nodes / 2: the size of the per-component arrays
    const int r = a.croot[c], len = a.cnt[r];
    int* lst = a.list + a.off[r];                          // [off, off + len) lies inside list: the scan summed these very counts
    int state = 1;
    double X[3] = {0, 0, 0}, err = 0.0;
    if (len > a.max_len) state = 3;
    else {
        for (int j = 1; j < len; ++j) {                    // ascending node order, whatever order the atomics left
            const int key = lst[j];
            int q = j - 1;
            while (q >= 0 && lst[q] > key) { lst[q + 1] = lst[q]; --q; }
            lst[q + 1] = key;
        }
        for (int j = 1; j < len; ++j) if (lst[j] / a.n == lst[j - 1] / a.n) state = 2;
        if (state == 1 && !a.tracks_only) state = tri_geometry(a, lst, len, X, err);
    }
    a.cstate[c] = state;
    float* res = a.cres + (long long)c * 4;
    res[0] = (float)X[0]; res[1] = (float)X[1]; res[2] = (float)X[2]; res[3] = (float)err;
}

// ------------------------------------------------------------------ 7. dense ids of the tracks of state 1, the per-track outputs, the counts
__global__ __launch_bounds__(TRI_SCAN_THREADS) void tri_number_kernel(TriArgs a) {
    __shared__ int sh[2 * TRI_SCAN_WAVES];
    __shared__ int per_state[8];
    const int C = a.head->components;
    if (threadIdx.x < 8) per_state[threadIdx.x] = 0;
    const int share = (C + TRI_SCAN_THREADS - 1) / TRI_SCAN_THREADS;
    const int beg = min((int)threadIdx.x * share, C), end = min(beg + share, C);
    int good = 0, unused = 0, total, t2;
    for (int c = beg; c < end; ++c) good += a.cstate[c] == 1;
    tri_block_scan(good, unused, total, t2, sh);           // (its barriers also publish the cleared per_state)
    for (int c = beg; c < end; ++c) {
        const int st = a.cstate[c];
        atomicAdd(per_state + (st & 7), 1);                // integer counts: the order of arrival changes nothing
        if (st != 1) { a.tid[c] = -1; continue; }
        a.tid[c] = good;                                   // good < total <= nodes / 2: the capacity of xyz, track_length, track_error
        a.track_length[good] = a.cnt[a.croot[c]];
        if (!a.tracks_only) {
            const float* res = a.cres + (long long)c * 4;
            a.xyz[(long long)good * 3] = res[0]; a.xyz[(long long)good * 3 + 1] = res[1]; a.xyz[(long long)good * 3 + 2] = res[2];
            a.track_error[good] = res[3];
        }
        ++good;
    }
    __syncthreads();
    if (threadIdx.x == 0) a.counts[0] = total;
    if (threadIdx.x < 8) a.counts[1 + threadIdx.x] = per_state[threadIdx.x];
}

// ------------------------------------------------------------------ 8. scatter
__global__ __launch_bounds__(TRI_THREADS) void tri_scatter_kernel(TriArgs a) {
    const int v = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (v >= a.nodes) return;
    const int r = a.root[v];
    int state = 0, id = -1;
    float x = __builtin_nanf(""), y = x, z = x;
    if (a.cnt[r] >= 2) {
        const int c = a.comp[r];
        state = a.cstate[c]; id = a.tid[c];
        if (state == 1 && !a.tracks_only) { const float* res = a.cres + (long long)c * 4; x = res[0]; y = res[1]; z = res[2]; }
    }
    a.node_state[v] = (unsigned char)state;
    a.track_id[v] = id;
    if (a.points3d) { float* p = a.points3d + (long long)v * 3; p[0] = x; p[1] = y; p[2] = z; }
}

// ------------------------------------------------------------------ the robust mode (lg_triangulate_robust): 6r. / 7r. / 8r. in the place of 6. / 7. / 8.
// Per component up to max_tracks rounds of: two-view hypotheses over the nodes that are left, an integer score per hypothesis (images with a passing node), the
// winner's per-image consensus, tri_geometry on that list.  A slot is (component, round): slot = component x max_tracks + round.
struct TriRobust {
    int nhyp, max_tracks;
    int* cons; int* nround;                                // per node: the consensus list of the running round (at the component's list offset); the round
                                                           // that took node v (-1: none)
    int* sstate; int* stid; int* slen; float* sres;        // per slot: round 0 its state, later rounds 1 or 0; dense id; consensus size; (X, Y, Z, error)
    int* outlier_counts;
};
constexpr int TRI_TAKEN = 1 << 30;                         // above every image index (images <= LG_MAX_ROWS = 2^21)

// what one lane of a wave wrote to the wave's LDS slice or to the component's lists, seen by the wave's other lanes: no other wave reads either
__device__ __forceinline__ void tri_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// hypothesis h of a round over L nodes: its index pair is number h of the Q = L (L - 1) / 2 pairs (i, j), i < j, in lexicographic order when Q <= nhyp, and
// number floor(h Q / nhyp) otherwise; the point is the linear start over the two observations in that order.  false: one image, a failed pivot, a non-finite X
__device__ __forceinline__ bool tri_hypothesis(const TriArgs& a, const float* xs, const float* ys, const int* img, int L, int nhyp, int h, double (&X)[3]) {
    const int Q = L * (L - 1) / 2;                         // L <= 1024: below 2^19
    const int p = Q <= nhyp ? h : (int)((long long)h * Q / nhyp);
    // row i of the pair triangle starts at i (2 L - i - 1) / 2: the root of that quadratic in fp64, then exact integer steps to the row that holds p
    const double w = 2.0 * L - 1.0;
    int i = (int)((w - sqrt(w * w - 8.0 * p)) * 0.5);
    i = max(0, min(i, L - 2));
    while (i > 0 && i * (2 * L - i - 1) / 2 > p) --i;
    while (i < L - 2 && (i + 1) * (2 * L - i - 2) / 2 <= p) ++i;
    const int j = min(p - i * (2 * L - i - 1) / 2 + i + 1, L - 1);
    const int ki = img[i], kj = img[j];
    if (ki == kj) return false;
    double S[6] = {0, 0, 0, 0, 0, 0}, B[3] = {0, 0, 0};
    tri_add_ray(a.rec[ki], xs[i], ys[i], S, B);
    tri_add_ray(a.rec[kj], xs[j], ys[j], S, B);
    return tri_solve3(S, B, X);
}

// ONE WAVE per component, four components per workgroup; no wave reads what another wrote, so there is no workgroup barrier and a wave may leave early.
// LDS: per wave 3 x max_len words (x, y, image index of the nodes that are left, in ascending node order); the node ids stay in the component's list.
__global__ __launch_bounds__(TRI_THREADS) void tri_robust_kernel(TriArgs a, TriRobust b) {
    extern __shared__ float tri_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int c = blockIdx.x * (TRI_THREADS / 64) + wave;
    if (c >= a.head->components) return;                   // components <= nodes / 2: the size of the per-component arrays
    float* xs = tri_lds + (size_t)wave * 3 * a.max_len;
    float* ys = xs + a.max_len;
    int* img = reinterpret_cast<int*>(ys + a.max_len);
    const int r = a.croot[c], len = a.cnt[r], n = a.n;
    int* lst = a.list + a.off[r];                          // [off, off + len) lies inside list and inside cons: the scan summed these very counts
    int* cons = b.cons + a.off[r];
    int* sstate = b.sstate + (long long)c * b.max_tracks;
    if (len > a.max_len) {
        if (lane < b.max_tracks) sstate[lane] = lane == 0 ? 3 : 0;
        return;
    }
    // ascending node order by rank (the nodes of a list are distinct, so the ranks are a permutation of [0, len)): whatever order the atomics left is gone
    for (int j = lane; j < len; j += 64) {
        const int key = lst[j];
        int rank = 0;
        for (int q = 0; q < len; ++q) rank += lst[q] < key;
        img[rank] = key;
    }
    tri_wave_sync();
    for (int j = lane; j < len; j += 64) {
        const int v = img[j];
        lst[j] = v; b.nround[v] = -1;
        xs[j] = a.kpts[(long long)v * 2]; ys[j] = a.kpts[(long long)v * 2 + 1]; img[j] = v / n;
    }
    tri_wave_sync();

    int L = len, rounds = 0;
    while (rounds < b.max_tracks) {
        // every lane scores its hypotheses h = lane, lane + 64, ...; q runs over the same LDS address in all lanes, and the image record's address is wave-uniform
        const int H = min(L * (L - 1) / 2, b.nhyp);
        unsigned best = 0;                                 // score << 16 | (0xFFFF - h); 0: no valid hypothesis (h <= 4095, so a valid key is never 0)
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int h = h0 + lane;
            double X[3] = {0, 0, 0};
            const bool valid = h < H && tri_hypothesis(a, xs, ys, img, L, b.nhyp, h, X);
            int score = 0, last = -1;                      // the nodes of one image are adjacent in the list
            for (int q = 0; q < L; ++q) {
                const int k = __builtin_amdgcn_readfirstlane(img[q]);
                double err;
                const bool pass = tri_obs_error(a.rec[k], xs[q], ys[q], X, err) && err <= a.max_err;
                if (pass && k != last) { ++score; last = k; }
            }
            if (valid) best = max(best, (unsigned)score << 16 | (0xFFFFu - (unsigned)h));
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
        int state = best == 0 ? 4 : (best >> 16) < 2 ? 6 : 1, m = 0;
        if (state == 1 && lane == 0) {
            double X[3], err = 0.0, low = 0.0;
            tri_hypothesis(a, xs, ys, img, L, b.nhyp, 0xFFFF - (int)(best & 0xFFFFu), X);       // the winner's point again: the same operations, the same bits
            int cur = -1, at = -1;                         // per image its passing node of smallest error; strict <: a tie keeps the lowest node
            for (int q = 0; q <= L; ++q) {
                const int k = q < L ? img[q] : -1;
                if (k != cur) {
                    if (at >= 0) { cons[m++] = lst[at]; img[at] |= TRI_TAKEN; }
                    cur = k; at = -1;
                }
                if (q < L && tri_obs_error(a.rec[k], xs[q], ys[q], X, err) && err <= a.max_err && (at < 0 || err < low)) { at = q; low = err; }
            }
            state = tri_geometry(a, cons, m, X, err);      // m >= 2 images passed under this very point
            if (state == 1) {
                const long long slot = (long long)c * b.max_tracks + rounds;
                b.slen[slot] = m;
                float* res = b.sres + slot * 4;
                res[0] = (float)X[0]; res[1] = (float)X[1]; res[2] = (float)X[2]; res[3] = (float)err;
                for (int j = 0; j < m; ++j) b.nround[cons[j]] = rounds;
                int keep = 0;                              // what is left moves up, in its order
                for (int q = 0; q < L; ++q) {
                    if (img[q] & TRI_TAKEN) continue;
                    lst[keep] = lst[q]; xs[keep] = xs[q]; ys[keep] = ys[q]; img[keep] = img[q];
                    ++keep;
                }
            }
        }
        state = __shfl(state, 0, 64); m = __shfl(m, 0, 64);
        if (lane == 0) sstate[rounds] = rounds == 0 ? state : (state == 1 ? 1 : 0);
        ++rounds;
        if (state != 1) break;                             // a failed round ends the component
        L -= m;
        if (L < 2) break;
        tri_wave_sync();
    }
    if (lane == 0) for (int k = rounds; k < b.max_tracks; ++k) sstate[k] = 0;
}

// 7r. dense ids over the slots of state 1 in ascending (component, round); counts as in tri_number (the failed components by their round-0 state); the nodes
// left over by the components whose round 0 succeeded, and the components with a second track
__global__ __launch_bounds__(TRI_SCAN_THREADS) void tri_number_robust_kernel(TriArgs a, TriRobust b) {
    __shared__ int sh[2 * TRI_SCAN_WAVES];
    __shared__ int per_state[8];
    __shared__ int extra[2];
    const int mt = b.max_tracks, slots = a.head->components * mt;      // components <= 2^20, max_tracks <= 4
    if (threadIdx.x < 8) per_state[threadIdx.x] = 0;
    if (threadIdx.x < 2) extra[threadIdx.x] = 0;
    const int share = (slots + TRI_SCAN_THREADS - 1) / TRI_SCAN_THREADS;
    const int beg = min((int)threadIdx.x * share, slots), end = min(beg + share, slots);
    int good = 0, unused = 0, total, t2;
    for (int s = beg; s < end; ++s) good += b.sstate[s] == 1;
    tri_block_scan(good, unused, total, t2, sh);           // (its barriers also publish the cleared counters)
    for (int s = beg; s < end; ++s) {
        const int c = s / mt, k = s - c * mt, st = b.sstate[s];
        if (k == 0 && st != 1) atomicAdd(per_state + (st & 7), 1);     // integer counts: the order of arrival changes nothing
        if (k == 0 && st == 1) atomicAdd(extra, a.cnt[a.croot[c]]);
        if (st != 1) { b.stid[s] = -1; continue; }
        if (k == 1) atomicAdd(extra + 1, 1);
        atomicAdd(extra, -b.slen[s]);
        b.stid[s] = good;                                  // good < total <= nodes / 2: a track has at least two nodes of its own
        a.track_length[good] = b.slen[s];
        const float* res = b.sres + (long long)s * 4;
        a.xyz[(long long)good * 3] = res[0]; a.xyz[(long long)good * 3 + 1] = res[1]; a.xyz[(long long)good * 3 + 2] = res[2];
        a.track_error[good] = res[3];
        ++good;
    }
    __syncthreads();
    if (threadIdx.x == 0) a.counts[0] = total;
    if (threadIdx.x < 8) a.counts[1 + threadIdx.x] = threadIdx.x == 1 ? total : per_state[threadIdx.x];
    if (threadIdx.x < 2) b.outlier_counts[threadIdx.x] = extra[threadIdx.x];
}

// 8r. a node of a component whose round 0 failed carries that state; otherwise its round's track, or state 8
__global__ __launch_bounds__(TRI_THREADS) void tri_scatter_robust_kernel(TriArgs a, TriRobust b) {
    const int v = blockIdx.x * TRI_THREADS + threadIdx.x;
    if (v >= a.nodes) return;
    const int r = a.root[v];
    int state = 0, id = -1;
    float x = __builtin_nanf(""), y = x, z = x;
    if (a.cnt[r] >= 2) {
        const long long first = (long long)a.comp[r] * b.max_tracks;
        state = b.sstate[first];
        if (state == 1) {
            const int k = b.nround[v];                     // -1, or a round that succeeded: below max_tracks
            if (k < 0) state = 8;
            else { id = b.stid[first + k]; const float* res = b.sres + (first + k) * 4; x = res[0]; y = res[1]; z = res[2]; }
        }
    }
    a.node_state[v] = (unsigned char)state;
    a.track_id[v] = id;
    float* p = a.points3d + (long long)v * 3;
    p[0] = x; p[1] = y; p[2] = z;
}

}  // namespace lg

using namespace lg;

namespace {

// the refusals of lg_triangulate behind its layout, in its order; `fn` starts every message
int tri_check(const char* fn, const lg_triangulate_io* io, const TriLayout& L) {
    const std::string name = std::string(fn) + ": ";
    const bool tracks_only = io->flags & LG_TRI_TRACKS_ONLY;
    const long long P = io->pairs, n = io->n;
    if (P < 0 || P * n >= (1LL << 31)) return set_error(LG_ERR_INVALID, name + "the pair count must not be negative and pairs x n must stay below 2^31");
    if (io->max_track_length < 2 || io->max_track_length > LG_TRI_MAX_TRACK_LENGTH)
        return set_error(LG_ERR_INVALID, name + "max_track_length must lie in [2, LG_TRI_MAX_TRACK_LENGTH]");
    if (!tracks_only && (!(io->max_reproj_error > 0.f) || !(io->max_reproj_error <= 3.0e18f)))
        return set_error(LG_ERR_INVALID, name + "max_reproj_error must be > 0 (and finite)");
    if (!tracks_only && (!(io->min_angle >= 0.f) || !(io->min_angle < 180.f))) return set_error(LG_ERR_INVALID, name + "min_angle must lie in [0, 180)");
    if (!io->counts || (P && (!io->index0 || !io->index1 || !io->status)) || (P && n && !io->matches0) || (L.nodes && (!io->track_id || !io->node_state || !io->track_length)) ||
        (!tracks_only && ((io->images && (!io->cameras || !io->poses)) || (L.nodes && (!io->kpts || !io->points3d || !io->xyz || !io->track_error)))))
        return set_error(LG_ERR_INVALID, name + "null pointer among kpts, index0, index1, matches0, cameras, poses, points3d, track_id, node_state, xyz, "
                                                "track_length, track_error, counts, status");
    return LG_OK;
}

TriArgs tri_bind(const lg_triangulate_io* io, const TriLayout& L) {
    const bool tracks_only = io->flags & LG_TRI_TRACKS_ONLY;
    char* ws = static_cast<char*>(io->workspace);
    TriArgs a{};
    a.pairs = io->pairs; a.n = io->n; a.images = io->images; a.nodes = (int)L.nodes; a.max_len = io->max_track_length;
    a.refine = (io->flags & LG_TRI_REFINE) ? 1 : 0; a.tracks_only = tracks_only ? 1 : 0;
    a.angle_test = !tracks_only && io->min_angle > 0.f; a.max_err = (double)io->max_reproj_error;
    a.cos_min = std::cos((double)io->min_angle * 3.141592653589793 / 180.0);
    a.kpts = io->kpts; a.num = io->num; a.index0 = io->index0; a.index1 = io->index1; a.matches0 = reinterpret_cast<const long long*>(io->matches0);
    a.cameras = io->cameras; a.poses = io->poses;
    auto ints = [&](long long at) { return reinterpret_cast<int*>(ws + at); };
    a.head = reinterpret_cast<TriHead*>(ws + L.head); a.rec = reinterpret_cast<TriImage*>(ws + L.rec);
    a.parent = ints(L.parent); a.root = ints(L.root); a.cnt = ints(L.cnt); a.off = ints(L.off); a.comp = ints(L.comp); a.cursor = ints(L.cursor); a.list = ints(L.list);
    a.croot = ints(L.croot); a.cstate = ints(L.cstate); a.tid = ints(L.tid); a.cres = reinterpret_cast<float*>(ws + L.cres);
    a.points3d = tracks_only ? nullptr : io->points3d; a.track_id = reinterpret_cast<long long*>(io->track_id); a.node_state = io->node_state;
    a.xyz = io->xyz; a.track_length = io->track_length; a.track_error = io->track_error; a.counts = io->counts; a.status = io->status;
    return a;
}

dim3 tri_blocks(long long items, int per_block = TRI_THREADS) { return dim3((unsigned)((items + per_block - 1) / per_block)); }

// launches 1 .. 5: every component's nodes in its list, in the order the atomics left
void tri_launch_lists(const TriArgs& a, const TriLayout& L, hipStream_t s) {
    const long long cells = (long long)a.pairs * a.n;
    const long long first = std::max<long long>(std::max<long long>(L.nodes, a.pairs), std::max<long long>(a.images, 1));
    hipLaunchKernelGGL(tri_init_kernel, tri_blocks(first), dim3(TRI_THREADS), 0, s, a);
    if (cells) hipLaunchKernelGGL(tri_union_kernel, tri_blocks(cells), dim3(TRI_THREADS), 0, s, a);
    if (L.nodes) hipLaunchKernelGGL(tri_flatten_kernel, tri_blocks(L.nodes), dim3(TRI_THREADS), 0, s, a);
    hipLaunchKernelGGL(tri_scan_kernel, dim3(1), dim3(TRI_SCAN_THREADS), 0, s, a);
    if (L.nodes) hipLaunchKernelGGL(tri_fill_kernel, tri_blocks(L.nodes), dim3(TRI_THREADS), 0, s, a);
}

}  // namespace

extern "C" {

int64_t lg_triangulate_workspace_bytes(int64_t images, int32_t n, uint32_t flags) {
    TriLayout L;
    return tri_layout(images, n, flags, L) ? -1 : L.total;
}

int lg_triangulate(const lg_triangulate_io* io, void* hip_stream) {
    if (!io) return set_error(LG_ERR_INVALID, "lg_triangulate: null io");
    TriLayout L;
    if (const char* why = tri_layout(io->images, io->n, io->flags, L)) return set_error(LG_ERR_INVALID, std::string("lg_triangulate: ") + why);
    if (const int rc = tri_check("lg_triangulate", io, L)) return rc;
    if (const int rc = check_workspace("lg_triangulate", "lg_triangulate_workspace_bytes", io->workspace, io->workspace_bytes, L.total)) return rc;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const TriArgs a = tri_bind(io, L);
    tri_launch_lists(a, L, s);
    if (L.tracks) hipLaunchKernelGGL(tri_tracks_kernel, tri_blocks(L.tracks), dim3(TRI_THREADS), 0, s, a);
    hipLaunchKernelGGL(tri_number_kernel, dim3(1), dim3(TRI_SCAN_THREADS), 0, s, a);
    if (L.nodes) hipLaunchKernelGGL(tri_scatter_kernel, tri_blocks(L.nodes), dim3(TRI_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

int64_t lg_triangulate_robust_workspace_bytes(int64_t images, int32_t n, int32_t max_tracks) {
    TriRobustLayout L;
    return tri_robust_layout(images, n, 0u, max_tracks, L) ? -1 : L.total;
}

int lg_triangulate_robust(const lg_triangulate_robust_io* rio, void* hip_stream) {
    if (!rio) return set_error(LG_ERR_INVALID, "lg_triangulate_robust: null io");
    const lg_triangulate_io* io = &rio->base;
    if (io->flags & LG_TRI_TRACKS_ONLY)
        return set_error(LG_ERR_INVALID, "lg_triangulate_robust: LG_TRI_TRACKS_ONLY is not accepted (the consensus needs the geometry; base.flags takes LG_TRI_REFINE only)");
    if (rio->num_hypotheses < 1 || rio->num_hypotheses > LG_TRI_MAX_HYPOTHESES)
        return set_error(LG_ERR_INVALID, "lg_triangulate_robust: num_hypotheses must lie in [1, LG_TRI_MAX_HYPOTHESES]");
    TriRobustLayout L;
    if (const char* why = tri_robust_layout(io->images, io->n, io->flags, rio->max_tracks, L)) return set_error(LG_ERR_INVALID, std::string("lg_triangulate_robust: ") + why);
    if (!rio->outlier_counts) return set_error(LG_ERR_INVALID, "lg_triangulate_robust: null pointer outlier_counts");
    if (const int rc = tri_check("lg_triangulate_robust", io, L.base)) return rc;
    if (const int rc = check_workspace("lg_triangulate_robust", "lg_triangulate_robust_workspace_bytes", io->workspace, io->workspace_bytes, L.total)) return rc;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const TriArgs a = tri_bind(io, L.base);
    char* ws = static_cast<char*>(io->workspace);
    auto ints = [&](long long at) { return reinterpret_cast<int*>(ws + at); };
    TriRobust b{};
    b.nhyp = rio->num_hypotheses; b.max_tracks = rio->max_tracks;
    b.cons = ints(L.cons); b.nround = ints(L.nround); b.sstate = ints(L.sstate); b.stid = ints(L.stid); b.slen = ints(L.slen);
    b.sres = reinterpret_cast<float*>(ws + L.sres); b.outlier_counts = rio->outlier_counts;
    tri_launch_lists(a, L.base, s);
    constexpr int waves = TRI_THREADS / 64;
    const size_t lds = (size_t)waves * 3 * a.max_len * sizeof(float);                    // 48 KB at max_track_length = 1024
    if (L.base.tracks) hipLaunchKernelGGL(tri_robust_kernel, tri_blocks(L.base.tracks, waves), dim3(TRI_THREADS), lds, s, a, b);
    hipLaunchKernelGGL(tri_number_robust_kernel, dim3(1), dim3(TRI_SCAN_THREADS), 0, s, a, b);
    if (L.base.nodes) hipLaunchKernelGGL(tri_scatter_robust_kernel, tri_blocks(L.base.nodes), dim3(TRI_THREADS), 0, s, a, b);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

}  // extern "C"
