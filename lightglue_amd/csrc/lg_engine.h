// lightglue_amd — the matcher engine's private state (struct lg_engine), shared by lg_engine.hip (workspace + forward),
// lg_weights.hip (weight re-packing) and lg_debug.hip (profiling, debug taps).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/lightglue_amd.h"
#include "lg_forward_plan.h"
#include "lg_host_call.h"
#include "lg_kernels.h"

#define TRY(x) do { int _rc = (x); if (_rc != LG_OK) return _rc; } while (0)

// kernel classes for lg_engine_profile_read (names: lg_debug.hip kProfNames)
enum { PC_PREP = 0, PC_GEMM_QKV_SELF, PC_ATTN_SELF, PC_GEMM_OUT, PC_GEMM_FFN1, PC_LN_GELU, PC_GEMM_FFN2, PC_GEMM_QKV_CROSS,
       PC_ATTN_CROSS, PC_ADAPTIVE, PC_ROWDOT, PC_GEMM_FINAL, PC_SIM, PC_ASSIGN, PC_TAIL, LG_PROF_NCLS };

namespace lg {

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };

// A device weight matrix [rows][K] in operand precision (+ the lo f16 plane for PREC_F16X3)
struct PackedW { void* hi = nullptr; void* lo = nullptr; };

inline size_t elem_size(int prec) { return prec == PREC_F32 ? 4 : 2; }

// One pass over the layout of a device arena; every piece starts on a 256-byte boundary.  base == nullptr is the MEASURING pass: nothing is
// assigned and `used` ends as the bytes the arena needs; with a base pointer the same sequence of take() calls CARVES it into the members.
struct Arena {
    char* base = nullptr; size_t used = 0;
    template <class T> void take(T*& member, size_t bytes) {
        used = (used + 255) & ~size_t(255);
        if (base) member = reinterpret_cast<T*>(base + used);
        used += bytes;
    }
};

// The weights of one transformer block, layer-major arrays; lg_engine::blocks[0] = SelfBlock, [1] = CrossBlock
struct BlockWeights {
    int Nout, n_qk_groups;                                    // q | k | v: 768, 2 (self);  qk | v: 512, 1 (cross)
    PackedW out, f1, f2;                                      // per-op path: out_proj / to_out, ffn.0, ffn.3
    float *b_qkv = nullptr, *b_out = nullptr, *b_f1 = nullptr, *b_f2 = nullptr;
    float *ln_g = nullptr, *ln_b = nullptr;                   // [L][512]
    char *tail_cat = nullptr, *tail_2 = nullptr;              // fused block tail (lg_tail.hip): fragment-packed [Wcat | planes] and W2 per layer
    float* b_cat = nullptr;                                   // ... and the folded bias
    char* qkv_p = nullptr; size_t qkv_layer_bytes = 0;        // fragment-packed q/k/v projection weights (lg_proj.hip)
};

}  // namespace lg

struct lg_engine {
    lg_config cfg{};
    int attn_prec = 0;
    std::map<std::string, lg::HostTensor> staged;
    bool weights_ready = false;
    // ---- device weights (layer-major arrays)
    void* w_arena = nullptr;
    lg::BlockWeights blocks[2] = {{768, 2}, {512, 1}};
    lg::PackedW w_in;
    float *b_in = nullptr, *b_final = nullptr;
    float *w_match = nullptr, *b_match = nullptr, *w_tok = nullptr, *b_tok = nullptr;  // [L][256], [L]
    float* Wr = nullptr;
    size_t tail_cat_layer_bytes = 0, tail_2_layer_bytes = 0;
    char* w_final_p = nullptr; size_t final_layer_bytes = 0;   // fragment-packed final projection weights (lg_proj.hip)
    lg::ForwardOptions opt;   // lg_engine_set_option, lg_engine_debug_stop_after (lg_forward_plan.h)
    long long* TAILDBG = nullptr; long long* TAILDBG2 = nullptr;   // shader-clock stamps of the kernel opt.tail_timing names
    int* CFLAGS = nullptr; int compact_epoch = 0; bool cflags_clean = false;   // compaction chunk flags [2B][cap / 128] + 1 error word (lg_adaptive.hip)
    // ---- workspace
    void* ws = nullptr; size_t ws_bytes = 0;
    int capB = 0, cap0 = 0, cap1 = 0;      // reserved
    int cur_cap0 = 0, cur_cap1 = 0, curB = 0;
    std::map<std::string, std::pair<void*, size_t>> bufs;
    float *X, *CTX, *MSG, *H1, *G, *COS, *SIN, *MD, *SIM, *LS, *LSNEG, *CONF, *MSCORE, *LSE_R, *LSE_C, *MAX0, *MAX1, *BBOX, *XIN, *CPM, *CPS, *CBV;
    int* CBI;
    void *Q, *K, *VT;
    int *IND, *DST, *LEN, *LEN_ORIG, *LEN_OLD, *ACTIVE, *FINAL_LAYER, *ARG0, *ARG1;
    int* RANGEF = nullptr;   // [B] range-guard flags (LG_FLAG_CHECK_FINITE), zeroed by init_state_kernel
    // gather path of the adaptive width (option "adapt_gather"): the second set of residual / rotary buffers, and which set each pair's rows are in
    float *X2 = nullptr, *COS2 = nullptr, *SIN2 = nullptr; int* XSEL = nullptr;
    // ---- per-kernel-class HIP-event timing (bench.py roofline leg)
    bool profiling = false, prof_open = false;
    int prof_only = -1;                // kernel class to time alone, -1 = every class
    struct ProfSpan { hipEvent_t a, b; int cls; };
    std::vector<ProfSpan> prof_pool;   // events, reused
    size_t prof_used = 0;
    double prof_ms[LG_PROF_NCLS] = {0};
    long long prof_cnt[LG_PROF_NCLS] = {0};
};

namespace lg {

// the layout of the weight arena (lg_weights.hip) and of the workspace for shape (B, c0, c1) (lg_engine.hip): one Arena pass each, measuring
// (base == nullptr) or carving into the engine's members; both return the bytes used
size_t weight_layout(lg_engine* e, char* base);
size_t workspace_layout(lg_engine* e, char* base, int B, int c0, int c1);

// brackets of one profiled launch group (lg_debug.hip)
int prof_begin(lg_engine* e, int cls, hipStream_t s);
int prof_end(lg_engine* e, hipStream_t s);

}  // namespace lg
