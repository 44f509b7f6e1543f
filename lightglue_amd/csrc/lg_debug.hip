// lightglue_amd — instrumentation of the matcher engine: per-kernel-class HIP-event profiling, the debug taps of the C ABI
// (lg_engine_debug_*) and the sustained matrix-core rate benchmark (lg_debug_mfma_sustained).
#include "lg_engine.h"

using namespace lg;

static const char* const kProfNames[LG_PROF_NCLS] = {"prep", "gemm_qkv_self", "attn_self", "gemm_out_proj", "gemm_ffn0", "ln_gelu", "gemm_ffn3_resid",
    "gemm_qkv_cross", "attn_cross", "adaptive", "rowdot", "gemm_final_proj", "sim", "assign", "fused_tail"};

namespace lg {

int prof_begin(lg_engine* e, int cls, hipStream_t s) {
    e->prof_open = e->profiling && (e->prof_only < 0 || e->prof_only == cls);   // "profile_only": time one class, leave the rest unbracketed
    if (!e->prof_open) return LG_OK;
    if (e->prof_used == e->prof_pool.size()) {
        lg_engine::ProfSpan sp{};
        HIPCHK(hipEventCreate(&sp.a)); HIPCHK(hipEventCreate(&sp.b));
        e->prof_pool.push_back(sp);
    }
    e->prof_pool[e->prof_used].cls = cls;
    HIPCHK(hipEventRecord(e->prof_pool[e->prof_used].a, s));
    return LG_OK;
}
int prof_end(lg_engine* e, hipStream_t s) {
    if (!e->prof_open) return LG_OK;
    e->prof_open = false;
    HIPCHK(hipEventRecord(e->prof_pool[e->prof_used].b, s));
    e->prof_used++;
    return LG_OK;
}

}  // namespace lg

namespace {

int prof_collect(lg_engine* e) {
    for (size_t i = 0; i < e->prof_used; ++i) {
        HIPCHK(hipEventSynchronize(e->prof_pool[i].b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->prof_pool[i].a, e->prof_pool[i].b));
        e->prof_ms[e->prof_pool[i].cls] += ms;
        e->prof_cnt[e->prof_pool[i].cls] += 1;
    }
    e->prof_used = 0;
    return LG_OK;
}

// matrix-core-dense spin: 2 waves per SIMD, 8 independent accumulators per wave (the pipe never waits), operands with
// pseudo-random bits (data that toggles: an all-zero spin runs ~15 % faster at the same power); block 0 reports its
// shader-clock span
__global__ __launch_bounds__(512) void mfma_spin_kernel(long long* cycles, int iters) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    const unsigned h = (threadIdx.x * 2654435761u + blockIdx.x * 40503u) * 12345u;
    u32x4 xa = {h ^ 0x3f803f80u, (h >> 3) | 0x3c003c00u, (h * 7u) & 0x3fff3fffu, (h * 13u) & 0x3fff3fffu};
    u32x4 xb = {(h * 3u) & 0x3fff3fffu, (h * 5u) & 0x3fff3fffu, (h * 11u) & 0x3fff3fffu, (h * 17u) & 0x3fff3fffu};
    f32x4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long t0 = clock64();
    for (int it = 0; it < iters; ++it) {
        asm volatile("" : "+v"(xa), "+v"(xb));
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, xa), __builtin_bit_cast(bf16x8_t, xb), acc[i], 0, 0, 0);
    }
    const long long t1 = clock64();
    float sacc = 0.f;
    for (int i = 0; i < 8; ++i) sacc += acc[i][0];
    // the LONGEST wave span: the arbiter issues oldest-first, so the older wave of a SIMD can finish in half the kernel's time
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(cycles), (unsigned long long)(t1 - t0));
    if (sacc == 12345.f) cycles[1] = 1;
}

}  // namespace

extern "C" {

int32_t lg_profile_num_classes(void) { return LG_PROF_NCLS; }
const char* lg_profile_class_name(int32_t cls) { return (cls >= 0 && cls < LG_PROF_NCLS) ? kProfNames[cls] : ""; }
int lg_engine_profile_enable(lg_engine* e, int32_t on) {
    if (!e) return set_error(LG_ERR_INVALID, "null engine");
    if (!on && e->profiling) { int rc = prof_collect(e); if (rc != LG_OK) return rc; }
    e->profiling = on != 0;
    return LG_OK;
}
int lg_engine_profile_read(lg_engine* e, double* ms, int64_t* count, int32_t n) {
    if (!e || !ms || !count || n < LG_PROF_NCLS) return set_error(LG_ERR_INVALID, "bad argument");
    int rc = prof_collect(e);
    if (rc != LG_OK) return rc;
    for (int i = 0; i < LG_PROF_NCLS; ++i) { ms[i] = e->prof_ms[i]; count[i] = e->prof_cnt[i]; e->prof_ms[i] = 0; e->prof_cnt[i] = 0; }
    return LG_OK;
}

int lg_engine_debug_stop_after(lg_engine* e, int32_t step) { if (!e) return set_error(LG_ERR_INVALID, "null engine"); e->opt.debug_stop = step; return LG_OK; }

/* What the matrix pipe SUSTAINS on this box: a dense v_mfma_f32_16x16x32_bf16 spin on every SIMD for ~25 ms (long enough for
 * the power management to settle).  tflops = achieved dense bf16 rate (the nominal 2.5 PFLOP/s assumes 2.4 GHz; under this load
 * the boxes of the pool hold 1.8 - 2.1 GHz), mhz = shader clock during the spin (s_memtime span of one wave / HIP-event time). */
int lg_debug_mfma_sustained(double* tflops, double* mhz, void* hip_stream) {
    if (!tflops || !mhz) return set_error(LG_ERR_INVALID, "null pointer");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    long long* d = nullptr;
    HIPCHK(hipMalloc(&d, 16));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    const int iters = 400000;
    hipLaunchKernelGGL(mfma_spin_kernel, dim3(256), dim3(512), 0, s, d, iters / 10);   // warm-up / clock ramp
    HIPCHK(hipMemsetAsync(d, 0, 16, s));
    HIPCHK(hipEventRecord(a, s));
    hipLaunchKernelGGL(mfma_spin_kernel, dim3(256), dim3(512), 0, s, d, iters);
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f; long long h[2] = {0, 0};
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    HIPCHK(hipMemcpy(h, d, 16, hipMemcpyDeviceToHost));
    (void)hipFree(d); (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    *mhz = ms > 0.f ? (double)h[0] / (ms * 1e3) : 0.0;
    *tflops = ms > 0.f ? 256.0 * 8.0 * iters * 8.0 * 16384.0 / (ms * 1e9) : 0.0;
    return LG_OK;
}

int lg_engine_debug_caps(lg_engine* e, int32_t* cap0, int32_t* cap1) {
    if (!e || !cap0 || !cap1) return set_error(LG_ERR_INVALID, "null argument");
    *cap0 = e->cur_cap0; *cap1 = e->cur_cap1;
    return LG_OK;
}

int lg_engine_debug_read(lg_engine* e, const char* name, void* host_dst, int64_t max_bytes, int64_t* nbytes_out) {
    if (!e || !name) return set_error(LG_ERR_INVALID, "null argument");
    auto it = e->bufs.find(name);
    if (it == e->bufs.end()) return set_error(LG_ERR_INVALID, std::string("unknown buffer '") + name + "'");
    if (nbytes_out) *nbytes_out = (int64_t)it->second.second;
    HIPCHK(hipDeviceSynchronize());
    if (host_dst && max_bytes > 0) {
        const size_t n = (size_t)max_bytes < it->second.second ? (size_t)max_bytes : it->second.second;
        HIPCHK(hipMemcpy(host_dst, it->second.first, n, hipMemcpyDeviceToHost));
    }
    return LG_OK;
}

}  // extern "C"
