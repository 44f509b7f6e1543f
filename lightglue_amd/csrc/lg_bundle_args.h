// lightglue_amd — what the two files of the bundle adjuster share (lg_bundle.hip, lg_bundle_focal.hip): the sizes, the device records, the kernels' argument
// blocks and the accessors of the state.  The definitions are in include/lightglue_amd.h (lg_bundle_adjust, lg_bundle_adjust_robust, lg_bundle_adjust_focal).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "lg_cholesky.h"
#include "../../include/lightglue_amd.h"

namespace lg {

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

__device__ __forceinline__ bool ba_adjusted(const BaArgs& a, int j) { const int c = a.tcnt[j]; return c >= 2 && c <= LG_BA_MAX_TRACK_LENGTH; }
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

// lg_bundle_focal.hip: the back substitution of lg_bundle_adjust_focal (ONE workgroup), enqueued on `s`
void ba_launch_backsolve_focal(const BaFocalArgs& a, hipStream_t s);

}  // namespace lg
