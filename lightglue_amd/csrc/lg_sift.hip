// lightglue_amd — SIFT helpers on the device (ref sift.py:17-56): the stand-alone RootSIFT transform (lg_rootsift; the engine applies the same device function
// where descriptors enter it, lg_pointwise.hip) and filter_dog_point (lg_sift_filter): duplicate removal, lowest angle, optional NMS, and a compaction of the
// kept indices in ascending order.  The SIFT detector itself is out of scope.
#include <string>

#include "lg_host_call.h"
#include "lg_side.h"
#include "../../include/lightglue_amd.h"

namespace lg {

// ------------------------------------------------------------------ RootSIFT: one wave per row, 4 rows per workgroup
struct RootSiftArgs { const void* src; int kind; long long rows; int dim; void* dst; int dst_f16; };

__global__ __launch_bounds__(256) void rootsift_kernel(RootSiftArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + wave;
    if (r >= a.rows) return;                       // uniform per wave
    const bool own = lane * 4 < a.dim;
    const long long at = r * a.dim + lane * 4;
    const f32x4 x = own ? load_desc4(a.src, a.kind, at) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 y = rootsift_row(x, lane, a.dim);
    if (!own) return;
    if (a.dst_f16) *reinterpret_cast<f16x4*>(static_cast<f16_t*>(a.dst) + at) = __builtin_convertvector(y, f16x4);   // v_cvt_f16_f32: round to nearest even, once
    else *reinterpret_cast<f32x4*>(static_cast<float*>(a.dst) + at) = y;
}

// ------------------------------------------------------------------ filter_dog_point (ref sift.py:17-50)
// Two int32 rasters per image, both cleared to 0 and raised by atomicMax on SIGNED integers:
//   M1[p] = bits of max(0, max s at p): for s >= 0 the order of the bit patterns is the order of the floats, and every s < 0 (sign bit: a negative integer)
//           loses against the initial 0, which is the reference's np.zeros buffer;
//   M2[p] = INF_BITS - bits of min |angle| among the points step 1 kept (0 = nothing entered = +inf, the reference's initial value).
// The NMS buffer of the reference (s of the kept points, 0 elsewhere) IS M1: wherever M1[p] > 0 some point attains it, and among those one attains the lowest
// angle, so a kept point with s == M1[p] exists; where M1[p] == 0 both hold 0.
struct SiftFilterArgs {
    const float* points; const float* scales; const float* angles; const float* scores; const int* num; const int* sizes;
    int images, n, max_h, max_w, radius;
    int* m1; int* m2; unsigned char* flags;     // [images][max_h * max_w] x 2, [images][n]
    long long* keep; int* counts;
};
constexpr int INF_BITS = 0x7F800000;

struct SiftPoint { bool live; int h, w, y, x; float s, a; long long pix; };
// detection i of image k: its pixel (ref :19, np.round = half to even = rintf in the default rounding mode), value and |angle|; live = counted and inside the image
__device__ __forceinline__ SiftPoint sift_point(const SiftFilterArgs& a, int k, int i) {
    SiftPoint p{};
    p.h = min(max(a.sizes[2 * k], 0), a.max_h); p.w = min(max(a.sizes[2 * k + 1], 0), a.max_w);      // a bad size cannot address outside the rasters
    if (i >= live_rows(a.num, k, a.n)) return p;
    const long long at = (long long)k * a.n + i;
    const float fy = rintf(a.points[2 * at + 1] - 0.5f), fx = rintf(a.points[2 * at] - 0.5f);
    if (!(fy >= 0.f && fy < (float)p.h && fx >= 0.f && fx < (float)p.w)) return p;                   // (NaN fails every comparison)
    p.y = (int)fy; p.x = (int)fx;
    p.s = (a.scores ? a.scores : a.scales)[at]; p.a = fabsf(a.angles[at]);
    p.pix = (long long)k * a.max_h * a.max_w + (long long)p.y * a.max_w + p.x;
    p.live = true;
    return p;
}

__global__ __launch_bounds__(256) void sift_max_kernel(SiftFilterArgs a) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const SiftPoint p = sift_point(a, k, i);
    if (p.live) atomicMax(a.m1 + p.pix, __float_as_int(p.s));
}
__global__ __launch_bounds__(256) void sift_angle_kernel(SiftFilterArgs a) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const SiftPoint p = sift_point(a, k, i);
    if (p.live && p.s == __int_as_float(a.m1[p.pix])) atomicMax(a.m2 + p.pix, INF_BITS - __float_as_int(p.a));
}
__global__ __launch_bounds__(256) void sift_flag_kernel(SiftFilterArgs a) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const SiftPoint p = sift_point(a, k, i);
    bool keep = false;
    if (p.live) {
        const float top = __int_as_float(a.m1[p.pix]);
        keep = p.s == top && p.a == __int_as_float(INF_BITS - a.m2[p.pix]);
        if (keep && a.radius > 0) {                   // max_pool2d pads with -inf: the window clipped to the image
            const int* m = a.m1 + (long long)k * a.max_h * a.max_w;
            const int y0 = max(p.y - a.radius, 0), y1 = min(p.y + a.radius, p.h - 1), x0 = max(p.x - a.radius, 0), x1 = min(p.x + a.radius, p.w - 1);
            int best = 0;                             // every entry is the pattern of a float >= 0: integer order
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) best = max(best, m[(long long)y * a.max_w + x]);
            keep = top == __int_as_float(best);
        }
    }
    a.flags[(long long)k * a.n + i] = keep ? 1 : 0;
}
// one workgroup per image: the kept indices in ascending order (a running block scan over the flags, 256 at a time), -1 behind them
__global__ __launch_bounds__(256) void sift_compact_kernel(SiftFilterArgs a) {
    const int k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char* flags = a.flags + (long long)k * a.n;
    long long* keep = a.keep + (long long)k * a.n;
    __shared__ int wsum[4];
    int base = 0;
    for (int i0 = 0; i0 < a.n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool f = i < a.n && flags[i] != 0;
        // compact_slot (lg_common.h) written out: through the helper hipcc allocates this kernel two more VGPRs (16 -> 18)
        const unsigned long long vote = __ballot(f);
        __syncthreads();                              // the previous round's wsum has been read
        if (lane == 0) wsum[wave] = __popcll(vote);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) { before += w < wave ? wsum[w] : 0; total += wsum[w]; }
        if (f) keep[base + before + __popcll(vote & ((1ull << lane) - 1ull))] = i;
        base += total;
    }
    for (int i = base + threadIdx.x; i < a.n; i += 256) keep[i] = -1;
    if (threadIdx.x == 0) a.counts[k] = base;
}

}  // namespace lg

using namespace lg;

extern "C" {

int lg_rootsift(const void* src, int32_t src_kind, int64_t rows, int32_t dim, void* dst, int32_t dst_f16, void* hip_stream) {
    if (src_kind != DESC_F32 && src_kind != DESC_F16 && src_kind != DESC_U8) return set_error(LG_ERR_INVALID, "lg_rootsift: src_kind must be 0 (float32), 1 (binary16) or 2 (uint8)");
    if (dim < 4 || dim > 256 || dim % 4) return set_error(LG_ERR_INVALID, "lg_rootsift: dim must be a multiple of 4 in [4, 256]");
    if (rows < 0 || rows > (1LL << 32)) return set_error(LG_ERR_INVALID, "lg_rootsift: rows must lie in [0, 2^32]");
    if (rows == 0) return LG_OK;
    if (!src || !dst) return set_error(LG_ERR_INVALID, "lg_rootsift: null pointer");
    const uintptr_t src_mask = src_kind == DESC_F32 ? 15 : src_kind == DESC_F16 ? 7 : 3, dst_mask = dst_f16 ? 7 : 15;
    if ((reinterpret_cast<uintptr_t>(src) & src_mask) || (reinterpret_cast<uintptr_t>(dst) & dst_mask))
        return set_error(LG_ERR_INVALID, "lg_rootsift: src / dst must be aligned to four of their elements (16 / 8 / 4 bytes)");
    const RootSiftArgs a{src, src_kind, (long long)rows, dim, dst, dst_f16 ? 1 : 0};
    hipLaunchKernelGGL(rootsift_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

int64_t lg_sift_filter_workspace_bytes(int32_t images, int32_t n, int32_t max_h, int32_t max_w) {
    SiftFilterLayout L;
    return sift_filter_layout(images, n, max_h, max_w, L) ? L.total : 0;
}

int lg_sift_filter(const float* points, const float* scales, const float* angles, const float* scores, const int32_t* num, const int32_t* sizes, int32_t images,
                   int32_t n, int32_t max_h, int32_t max_w, int32_t nms_radius, void* workspace, int64_t workspace_bytes, int64_t* keep, int32_t* counts,
                   void* hip_stream) {
    SiftFilterLayout L;
    if (!sift_filter_layout(images, n, max_h, max_w, L))
        return set_error(LG_ERR_INVALID, "lg_sift_filter: images in [1, 65535], n in [0, 2^24], max_h x max_w in [1, 2^31 - 1] pixels");
    if (nms_radius < 0 || nms_radius > 64) return set_error(LG_ERR_INVALID, "lg_sift_filter: nms_radius must lie in [0, 64]");
    if (!sizes || !counts || (n && (!points || !scales || !angles || !keep))) return set_error(LG_ERR_INVALID, "lg_sift_filter: null pointer");
    if (const int rc = check_workspace("lg_sift_filter", "lg_sift_filter_workspace_bytes", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(workspace);
    const SiftFilterArgs a{points, scales, angles, scores, num, sizes, images, n, max_h, max_w, nms_radius,
                           reinterpret_cast<int*>(ws + L.m1), reinterpret_cast<int*>(ws + L.m2), reinterpret_cast<unsigned char*>(ws + L.flags),
                           reinterpret_cast<long long*>(keep), counts};
    if (n > 0) {
        HIPCHK(hipMemsetAsync(ws, 0, (size_t)L.flags, s));
        const dim3 grid((n + 255) / 256, images);
        hipLaunchKernelGGL(sift_max_kernel, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(sift_angle_kernel, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(sift_flag_kernel, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(sift_compact_kernel, dim3(images), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

}  // extern "C"
