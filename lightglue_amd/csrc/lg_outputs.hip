// lightglue_amd — the first and the last kernel of every matcher forward (state initialisation; outputs in the reference's dtypes, the
// packed wire row, the per-pair status) and the inverse of the wire row, lg_unpack_wire (ref lightglue.py:535-540, :593-629).
#include "../../include/lightglue_amd.h"
#include "lg_kernels.h"

namespace lg {
namespace {

// keypoints of side `image` of a pair: the live rows of the image it reads (indexed inputs: num is per image); 0 on both sides for a pair whose index is out of range
__device__ __forceinline__ int count(const int* num, const PairIndex& px, int pair, int image, int n) {
    const int src = source_image(px, pair, image);
    return src < 0 ? 0 : live_rows(num, src, n);
}

__global__ void init_state_kernel(InitStateArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, B = a.B, n0 = a.n0, n1 = a.n1;
    if (a.range_flag && i < B) a.range_flag[i] = 0;
    if (a.xsel && i < B) a.xsel[i] = 0;
    if (a.device_err && i == 0) *a.device_err = 0;
    if (a.len && i < B) {
        const int l0 = count(a.num0, a.px, i, 0, n0), l1 = count(a.num1, a.px, i, 1, n1);
        a.len[2 * i] = l0; a.len[2 * i + 1] = l1; a.len_orig[2 * i] = l0; a.len_orig[2 * i + 1] = l1;
        a.len_old[2 * i] = -1; a.len_old[2 * i + 1] = -1;
        // a pair with an empty image never enters the layer loop: stop = 1, empty result (ref :539-540, :568-588)
        const int live = l0 > 0 && l1 > 0;
        a.active[i] = live; a.final_layer[i] = live ? a.L - 1 : 0;
    }
    // prune counters start at 1 for every keypoint (ref :535-536); padding rows of a ragged batch get 0
    if (a.prune0) for (long long k = i; k < (long long)B * n0; k += (long long)gridDim.x * blockDim.x) a.prune0[k] = (int)(k % n0) < count(a.num0, a.px, (int)(k / n0), 0, n0);
    if (a.prune1) for (long long k = i; k < (long long)B * n1; k += (long long)gridDim.x * blockDim.x) a.prune1[k] = (int)(k % n1) < count(a.num1, a.px, (int)(k / n1), 1, n1);
}
__global__ __launch_bounds__(256) void write_outputs_kernel(OutArgs a) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int stop = a.final_layer ? a.final_layer[b] + 1 : a.stop_const;
    int* wrow = a.wire ? a.wire + (long long)b * a.wire_stride : nullptr;
    const int wp = 2 * a.n0 + 2 * a.n1 + 2;   // first element of the wire row's prune block
    if (i == 0) {
        const int status = (a.device_err && *a.device_err) ? LG_ERR_DEVICE : source_image(a.px, b, 0) < 0 ? LG_ERR_INDEX
                           : ((a.range_flag && a.range_flag[b]) ? LG_ERR_RANGE : LG_OK);
        a.stop[b] = stop;
        if (a.stop_64) a.stop_64[b] = stop;
        if (wrow) { wrow[wp - 2] = stop; wrow[wp - 1] = status; }
        if (a.status) a.status[b] = status;
    }
    if (i < a.n0) {
        const long long k = (long long)b * a.n0 + i;
        const int m = a.m0[k];
        const float fill = i < count(a.num0, a.px, b, 0, a.n0) ? (float)a.L : 0.f;
        if (a.m0_64) a.m0_64[k] = m;
        if (a.prune0_64) a.prune0_64[k] = a.prune0[k];
        if (a.prune0_f) a.prune0_f[k] = fill;
        if (wrow) { wrow[i] = m; wrow[a.n0 + i] = __float_as_int(a.s0[k]); wrow[wp + i] = a.wire_prune ? a.prune0[k] : __float_as_int(fill); }
    }
    if (i < a.n1) {
        const long long k = (long long)b * a.n1 + i;
        const int m = a.m1[k];
        const float fill = i < count(a.num1, a.px, b, 1, a.n1) ? (float)a.L : 0.f;
        if (a.m1_64) a.m1_64[k] = m;
        if (a.prune1_64) a.prune1_64[k] = a.prune1[k];
        if (a.prune1_f) a.prune1_f[k] = fill;
        if (wrow) { wrow[2 * a.n0 + i] = m; wrow[2 * a.n0 + a.n1 + i] = __float_as_int(a.s1[k]); wrow[wp + a.n0 + i] = a.wire_prune ? a.prune1[k] : __float_as_int(fill); }
    }
    if (a.matches_64 && i < 2 * a.kmax && (i >> 1) < a.n_matches[b]) {
        const long long k = (long long)b * a.kmax * 2 + i;
        a.matches_64[k] = a.matches[k];
    }
}
// inverse of the wire row on gathered rows (lg_unpack_wire): one workgroup of 1024 threads per gathered row.  Besides the permutation / widening it
// builds the reference's sorted match list (ref :593-602: indices of matches0 > -1 in ascending order, their partners, their scores) by ballot +
// popcount prefix over the row, and the [3][pairs_out] host block (stop | n_matches | status).
struct UnpackArgs {
    const int* wire; long long stride; int n0, n1, pairs_out, kmax; const int* order;
    long long* m0; long long* m1; long long* stop; float* s0; float* s1;
    long long* p0_64; long long* p1_64; float* p0_f; float* p1_f;
    long long* matches; float* mscores; int* info;
};
__global__ __launch_bounds__(1024) void unpack_wire_kernel(UnpackArgs a) {
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n0 = a.n0, n1 = a.n1;
    const int* row = a.wire + (long long)r * a.stride;
    const long long d = a.order ? a.order[r] : r;
    if (d < 0 || d >= a.pairs_out) return;      // a padding row of a short shard
    const int wp = 2 * n0 + 2 * n1 + 2;
    __shared__ int sh_cnt[16];
    int base = 0;                                // matches found in the chunks before this one (the same value in every thread)
    for (int i0 = 0; i0 < n0; i0 += 1024) {
        const int i = i0 + tid;
        int m = -1; float sc = 0.f;
        if (i < n0) {
            m = row[i]; sc = __int_as_float(row[n0 + i]);
            if (a.m0) a.m0[d * n0 + i] = m;
            if (a.s0) a.s0[d * n0 + i] = sc;
            if (a.p0_64) a.p0_64[d * n0 + i] = row[wp + i];
            if (a.p0_f) a.p0_f[d * n0 + i] = __int_as_float(row[wp + i]);
        }
        const bool valid = m > -1;
        const unsigned long long bal = __ballot(valid);
        if (lane == 0) sh_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = sh_cnt[w]; if (w < wv) before += c; total += c; }
        if (valid && a.matches) {
            const long long k = d * a.kmax + before + __popcll(bal & ((1ull << lane) - 1ull));
            a.matches[2 * k] = i; a.matches[2 * k + 1] = m;
            if (a.mscores) a.mscores[k] = sc;
        }
        base += total;
        __syncthreads();                         // sh_cnt is rewritten by the next chunk
    }
    for (int i = tid; i < n1; i += 1024) {
        if (a.m1) a.m1[d * n1 + i] = row[2 * n0 + i];
        if (a.s1) a.s1[d * n1 + i] = __int_as_float(row[2 * n0 + n1 + i]);
        if (a.p1_64) a.p1_64[d * n1 + i] = row[wp + n0 + i];
        if (a.p1_f) a.p1_f[d * n1 + i] = __int_as_float(row[wp + n0 + i]);
    }
    if (tid == 0) {
        if (a.stop) a.stop[d] = row[wp - 2];
        if (a.info) { a.info[d] = row[wp - 2]; a.info[a.pairs_out + d] = base; a.info[2 * a.pairs_out + d] = row[wp - 1]; }
    }
}

}  // namespace

hipError_t launch_init_state(const InitStateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(init_state_kernel, dim3(64), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_write_outputs(const OutArgs& a, hipStream_t s) {
    int span = a.n0 > a.n1 ? a.n0 : a.n1; if (2 * a.kmax > span) span = 2 * a.kmax; if (span < 1) span = 1;
    hipLaunchKernelGGL(write_outputs_kernel, dim3((span + 255) / 256, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace lg

using namespace lg;

extern "C" {

int lg_unpack_wire(const lg_unpack_io* io, void* hip_stream) {
    if (!io || io->rows < 0 || io->n0 < 0 || io->n1 < 0 || io->pairs_out < 0) return set_error(LG_ERR_INVALID, "lg_unpack_wire: bad argument");
    if (io->rows == 0 || io->pairs_out == 0) return LG_OK;    // an empty gather (world of one, empty batch) is a no-op
    if (!io->wire || io->wire_stride < LG_WIRE_WIDTH(io->n0, io->n1)) return set_error(LG_ERR_INVALID, "lg_unpack_wire: null wire or wire_stride < LG_WIRE_WIDTH(n0, n1)");
    if (io->n0 > LG_MAX_KEYPOINTS || io->n1 > LG_MAX_KEYPOINTS) return set_error(LG_ERR_INVALID, "lg_unpack_wire: more than LG_MAX_KEYPOINTS keypoints");
    UnpackArgs a{};
    a.wire = io->wire; a.stride = io->wire_stride; a.n0 = io->n0; a.n1 = io->n1; a.pairs_out = io->pairs_out;
    a.kmax = io->n0 < io->n1 ? io->n0 : io->n1; a.order = io->order;
    a.m0 = (long long*)io->matches0; a.m1 = (long long*)io->matches1; a.stop = (long long*)io->stop; a.s0 = io->scores0; a.s1 = io->scores1;
    if (io->with_prune) { a.p0_64 = (long long*)io->prune0_i64; a.p1_64 = (long long*)io->prune1_i64; }
    else { a.p0_f = io->prune0_f32; a.p1_f = io->prune1_f32; }
    a.matches = (long long*)io->matches; a.mscores = io->match_scores; a.info = io->info;
    hipLaunchKernelGGL(unpack_wire_kernel, dim3(io->rows), dim3(1024), 0, static_cast<hipStream_t>(hip_stream), a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

}  // extern "C"
