// lightglue_amd — how one side of a call enters the engine, written once for every kernel that reads a forward's inputs: the normalised keypoint and its Fourier
// phase (ref lightglue.py:32-43, :76-81; prep_kernel in lg_pointwise.hip and the fused first projection, FirstRows in lg_proj.hip), descriptor rows in their
// storage format (fp32, binary16, uint8: the kinds are lg_forward_plan.h's DESC_*, host-visible) and the RootSIFT transform (ref sift.py:53-56; prep_kernel
// and the stand-alone rootsift_kernel, lg_sift.hip).
#pragma once
#include "lg_forward_plan.h"
#include "lg_kernels.h"

namespace lg {

// ---- the keypoint of input row `in_row` (= simg * sd.n + r, simg the image the segment reads) normalised by the image size or, without one, by the bounding
// box of the segment's keypoints (ref :32-43); with pos_dim == 4 its scale and orientation behind it (ref :495-501).  kn[2], kn[3] stay unset otherwise.
__device__ __forceinline__ void normalised_keypoint(const PrepArgs& a, const PrepSide& sd, int seg, long long simg, long long in_row, float (&kn)[4]) {
    const float* kp = sd.kpts + in_row * 2;
    float sx, sy;
    if (sd.size) { sx = sd.size[simg * 2]; sy = sd.size[simg * 2 + 1]; }
    else { const float* bb = a.bbox + seg * 4; sx = 1.f + bb[2] - bb[0]; sy = 1.f + bb[3] - bb[1]; }
    const float scale = fmaxf(sx, sy) / 2.f;          // ref :41
    kn[0] = (kp[0] - sx / 2.f) / scale;               // ref :40, :42
    kn[1] = (kp[1] - sy / 2.f) / scale;
    if (a.pos_dim == 4) { kn[2] = sd.scales[in_row]; kn[3] = sd.oris[in_row]; }
}
// the phase of frequency f (0 .. 31, shared by all heads; ref :78-79): the caller stores its cosf and sinf
__device__ __forceinline__ float fourier_phase(const PrepArgs& a, const float (&kn)[4], int f) {
    float p = 0.f;
    for (int c = 0; c < a.pos_dim; ++c) p += kn[c] * a.Wr[f * a.pos_dim + c];
    return p;
}

typedef unsigned char u8x4 __attribute__((ext_vector_type(4)));

// ---- uint8 -> fp32 of descriptors that are STORED as bytes (LG_FLAG_DESC0_U8 / _DESC1_U8; COLMAP / OpenCV SIFT): v_cvt_f32_ubyte0..3, exact (0 .. 255)
__device__ __forceinline__ f32x4 widen4_u8(const u8x4& b) { return __builtin_convertvector(b, f32x4); }

// four consecutive values at element `at` (a multiple of 4) of a descriptor array in storage format `kind`: one 16- / 8- / 4-byte load, widened exactly
__device__ __forceinline__ f32x4 load_desc4(const void* base, int kind, long long at) {
    if (kind == DESC_U8) return widen4_u8(*reinterpret_cast<const u8x4*>(static_cast<const unsigned char*>(base) + at));
    if (kind == DESC_F16) return widen4_f16(*reinterpret_cast<const f16x4*>(static_cast<const f16_t*>(base) + at));
    return *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + at);
}

// max(v, eps) as torch.clamp(min = eps) has it: a NaN stays a NaN
__device__ __forceinline__ float clamp_min(float v, float eps) { return v < eps ? eps : v; }

// RootSIFT of one row of d <= 256 values held by one wave: lane l holds x[4l .. 4l + 3], lanes past the row hold zeros and get zeros back.  Every lane of the
// wave must call it.  L1-normalise, clip, sqrt, L2-normalise with eps = 1e-6 (ref sift.py:53-56: F.normalize(p = 1), clip_(min = eps).sqrt_(),
// F.normalize(p = 2)); IEEE division and sqrtf (the build has no fast-math).  The sums are xor butterflies: one fixed order, every lane the same total.
__device__ __forceinline__ f32x4 rootsift_row(const f32x4& x, int lane, int d) {
    constexpr float eps = 1e-6f;
    const float n1 = clamp_min(wave_sum(fabsf(x[0]) + fabsf(x[1]) + fabsf(x[2]) + fabsf(x[3])), eps);
    f32x4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = sqrtf(clamp_min(x[i] / n1, eps));
    const bool own = lane * 4 < d;     // the clipped sqrt(eps) of the lanes past the row is not part of the row's norm
    // (explicit fmaf chain: both kernels that inline this must round alike, whatever the compiler would contract)
    const float sq = fmaf(y[3], y[3], fmaf(y[2], y[2], fmaf(y[1], y[1], y[0] * y[0])));
    const float n2 = clamp_min(sqrtf(wave_sum(own ? sq : 0.f)), eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = own ? y[i] / n2 : 0.f;
    return y;
}

}  // namespace lg
