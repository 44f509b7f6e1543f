// lightglue_amd — matcher weights: host-side conversion to the operand precisions, the packers, and the weight arena
// (lg_engine_set_weight / lg_engine_finalize_weights).  Replaces LightGlue.__init__ weight handling (ref lightglue.py:376-437).
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "lg_engine.h"

using namespace lg;

namespace {

// ---- host-side fp32 -> 16-bit conversions (round to nearest even)
inline uint16_t f32_to_bf16(float f) {
    uint32_t u; std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline uint16_t f32_to_f16(float f) {
    uint32_t x; std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0u));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to >= 65520 -> inf
    if (x < 0x33000001u) return (uint16_t)sign;               // rounds to zero
    int e = (int)(x >> 23) - 127;
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    int shift;
    uint32_t half_e;
    if (e < -14) { shift = 13 + (-14 - e); half_e = 0; } else { shift = 13; half_e = (uint32_t)(e + 15); }
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (r & 1u))) r++;
    // r includes the implicit bit for normals: (half_e << 10) + (r - 0x400) == ((half_e - 1) << 10) + r
    const uint32_t out = half_e ? (((half_e - 1u) << 10) + r) : r;
    return (uint16_t)(sign | out);
}

inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = sign;
        else { int sh = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++sh; } u = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((mm & 0x3ffu) << 13); }
    } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
    else u = sign | ((e + 112u) << 23) | (m << 13);
    float f; std::memcpy(&f, &u, 4); return f;
}

// element idx of a host matrix in operand precision; split f16: hi = f16(v), and lo = f16(v - hi) in the lo plane
inline void store_elem(int prec, void* hi, void* lo, size_t idx, float v) {
    if (prec == PREC_F32) static_cast<float*>(hi)[idx] = v;
    else if (prec == PREC_BF16) static_cast<uint16_t*>(hi)[idx] = f32_to_bf16(v);
    else {
        const uint16_t h = f32_to_f16(v);
        static_cast<uint16_t*>(hi)[idx] = h;
        if (prec_is_split(prec)) static_cast<uint16_t*>(lo)[idx] = f32_to_f16(v - f16_to_f32(h));
    }
}

// pack a [rows][K] fp32 host matrix into operand precision at device memory (split f16: hi and lo planes)
int upload_packed(int prec, const float* src, size_t n, PackedW& dst, size_t elem_offset) {
    const size_t es = elem_size(prec);
    std::vector<char> hi(n * es), lo(prec_is_split(prec) ? n * es : 0);
    for (size_t i = 0; i < n; ++i) store_elem(prec, hi.data(), lo.data(), i, src[i]);
    HIPCHK(hipMemcpy(static_cast<char*>(dst.hi) + elem_offset * es, hi.data(), n * es, hipMemcpyHostToDevice));
    if (prec_is_split(prec)) HIPCHK(hipMemcpy(static_cast<char*>(dst.lo) + elem_offset * es, lo.data(), n * es, hipMemcpyHostToDevice));
    return LG_OK;
}

// MFMA-fragment order (lg_kernels.h TailArgs): plane-major (hi, then lo), then [n-tile][k-chunk][lane][EPC]
int upload_fragment_packed(int prec, const std::vector<double>& W, int rows, int K, char* dst) {
    const size_t es = elem_size(prec), n = (size_t)rows * K;
    const int EPC = prec == PREC_F32 ? 4 : 8, KC = 4 * EPC, NKC = K / KC, NT = rows / 16;
    std::vector<char> buf(n * es * (prec_is_split(prec) ? 2 : 1));
    for (int nt = 0; nt < NT; ++nt)
        for (int kc = 0; kc < NKC; ++kc)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < EPC; ++j) {
                    const float v = (float)W[(size_t)(nt * 16 + (lane & 15)) * K + kc * KC + (lane >> 4) * EPC + j];
                    store_elem(prec, buf.data(), buf.data() + n * es, ((size_t)(nt * NKC + kc) * 64 + lane) * EPC + j, v);
                }
    HIPCHK(hipMemcpy(dst, buf.data(), buf.size(), hipMemcpyHostToDevice));
    return LG_OK;
}

// Row order of the fragment-packed q/k/v projection weights (lg_proj_body.h pj_tile): n-tile t, MFMA row i -> packed column
// ([group][head][64]).  The n_qk leading groups of 16 tiles each (q, k / qk) are dealt in PAIRS of adjacent tiles whose 32 rows are
// interleaved in blocks of 4 — tile 2p + e, row 4g + r <- channel 32p + 8g + 4e + r — so that a lane of the transposed MFMA form
// ends with 8 consecutive channels (one 16-byte store per plane); v tiles keep the natural order.
std::vector<double> proj_row_permutation(const std::vector<float>& pw, int nout, int n_qk_groups, int K) {
    std::vector<double> out((size_t)nout * K);
    for (int t = 0; t < nout / 16; ++t)
        for (int i = 0; i < 16; ++i) {
            int col = t * 16 + i;
            if (t < 16 * n_qk_groups) {
                const int group = t / 16, tg = t % 16;
                col = group * 256 + 32 * (tg / 2) + 8 * (i >> 2) + 4 * (tg % 2) + (i & 3);
            }
            for (int k = 0; k < K; ++k) out[(size_t)(t * 16 + i) * K + k] = pw[(size_t)col * K + k];
        }
    return out;
}

const HostTensor* find(const lg_engine* e, const std::string& name, std::initializer_list<int64_t> shape, std::string& err) {
    auto it = e->staged.find(name);
    if (it == e->staged.end()) { err = "missing weight '" + name + "'"; return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) { err = "bad shape for '" + name + "'"; return nullptr; }
    return &it->second;
}

}  // namespace

namespace lg {

// The weight arena, described once: measured with base == nullptr, carved into the engine's members otherwise (see Arena).
// Every size depends on the engine's configuration alone, so both passes take the same pieces.
size_t weight_layout(lg_engine* e, char* base) {
    const size_t L = e->cfg.n_layers, D = 256, Din = e->cfg.input_dim, es = elem_size(e->cfg.precision);
    const bool split = prec_is_split(e->cfg.precision);
    const size_t planes = split ? 2 : 1;
    Arena ar{base};
    auto takew = [&](PackedW& w, size_t elems) { ar.take(w.hi, elems * es); if (split) ar.take(w.lo, elems * es); };
    auto takef = [&](float*& p, size_t n) { ar.take(p, n * 4); };
    takew(e->w_in, D * Din);
    for (BlockWeights& b : e->blocks) { takew(b.out, L * D * D); takew(b.f1, L * 512 * 512); takew(b.f2, L * D * 512); }
    takef(e->b_in, D);
    for (BlockWeights& b : e->blocks) { takef(b.b_qkv, L * b.Nout); takef(b.b_out, L * D); takef(b.b_f1, L * 512); takef(b.b_f2, L * D); }
    takef(e->b_final, L * D);
    for (BlockWeights& b : e->blocks) { takef(b.ln_g, L * 512); takef(b.ln_b, L * 512); }
    takef(e->w_match, L * D); takef(e->b_match, L); takef(e->w_tok, L * D); takef(e->b_tok, L); takef(e->Wr, 32 * 4);
    // fragment-packed weights: hi plane then lo plane per layer
    e->tail_cat_layer_bytes = 512 * 512 * es * planes; e->tail_2_layer_bytes = 256 * 512 * es * planes;
    for (BlockWeights& b : e->blocks) { ar.take(b.tail_cat, L * e->tail_cat_layer_bytes); ar.take(b.tail_2, L * e->tail_2_layer_bytes); }
    for (BlockWeights& b : e->blocks) takef(b.b_cat, L * 512);
    for (BlockWeights& b : e->blocks) { b.qkv_layer_bytes = b.Nout * D * es * planes; ar.take(b.qkv_p, L * b.qkv_layer_bytes); }
    e->final_layer_bytes = D * D * es * planes; ar.take(e->w_final_p, L * e->final_layer_bytes);
    return ar.used;
}

}  // namespace lg

extern "C" {

int lg_engine_set_weight(lg_engine* e, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    if (!e || !name || !host_data || ndim < 0 || ndim > 4) return set_error(LG_ERR_INVALID, "bad argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host_data, host_data + n);
    e->staged[name] = std::move(t);
    e->weights_ready = false;
    return LG_OK;
}

int lg_engine_finalize_weights(lg_engine* e) {
    if (!e) return set_error(LG_ERR_INVALID, "null engine");
    const int L = e->cfg.n_layers, D = 256, Din = e->cfg.input_dim, prec = e->cfg.precision;
    const int pos_dim = 2 + 2 * (e->cfg.add_scale_ori ? 1 : 0);
    const size_t total = weight_layout(e, nullptr);
    HIPCHK(hipDeviceSynchronize());   // weights may be in use by forwards still running on any stream
    if (e->w_arena) { HIPCHK(hipFree(e->w_arena)); e->w_arena = nullptr; }
    HIPCHK(hipMalloc(&e->w_arena, total));
    HIPCHK(hipMemset(e->w_arena, 0, total));
    if (weight_layout(e, static_cast<char*>(e->w_arena)) > total) return set_error(LG_ERR_STATE, "weight arena carve overflow");

    std::string err;
    auto up_f32 = [&](float* dst, const float* src, size_t n) -> int { HIPCHK(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice)); return LG_OK; };
#define NEED(var, name, ...) const HostTensor* var = find(e, name, {__VA_ARGS__}, err); if (!var) return set_error(LG_ERR_INVALID, err)
    {
        NEED(wr, "posenc.Wr.weight", 32, pos_dim);
        TRY(up_f32(e->Wr, wr->data.data(), 32 * (size_t)pos_dim));
    }
    if (Din != D) {
        NEED(w, "input_proj.weight", D, Din); NEED(b, "input_proj.bias", D);
        TRY(upload_packed(prec, w->data.data(), (size_t)D * Din, e->w_in, 0));
        TRY(up_f32(e->b_in, b->data.data(), D));
    }
    for (int i = 0; i < L; ++i) {
        const std::string prefix[2] = {"transformers." + std::to_string(i) + ".self_attn.", "transformers." + std::to_string(i) + ".cross_attn."};
        const std::string &s = prefix[0], &c = prefix[1];
        const char* const out_name[2] = {"out_proj", "to_out"};
        BlockWeights &sb = e->blocks[0], &cb = e->blocks[1];
        {   // Wqkv: reference channel = head*192 + d*3 + {q,k,v} (ref :166-167) -> packed column = which*256 + head*64 + d
            NEED(w, s + "Wqkv.weight", 768, D); NEED(b, s + "Wqkv.bias", 768);
            std::vector<float> pw((size_t)768 * D), pb(768);
            for (int which = 0; which < 3; ++which) for (int h = 0; h < 4; ++h) for (int d = 0; d < 64; ++d) {
                const int src = h * 192 + d * 3 + which, dst = which * 256 + h * 64 + d;
                std::memcpy(&pw[(size_t)dst * D], &w->data[(size_t)src * D], D * 4);
                pb[dst] = b->data[src];
            }
            TRY(upload_fragment_packed(prec, proj_row_permutation(pw, 768, sb.n_qk_groups, D), 768, D, sb.qkv_p + (size_t)i * sb.qkv_layer_bytes));
            TRY(up_f32(sb.b_qkv + (size_t)i * 768, pb.data(), 768));
        }
        for (int blk = 0; blk < 2; ++blk) {
            const std::string& p = prefix[blk];
            BlockWeights& bw = e->blocks[blk];
            NEED(wo, p + out_name[blk] + ".weight", D, D); NEED(bo, p + out_name[blk] + ".bias", D);
            NEED(w0, p + "ffn.0.weight", 512, 512); NEED(b0, p + "ffn.0.bias", 512);
            NEED(g, p + "ffn.1.weight", 512); NEED(be, p + "ffn.1.bias", 512);
            NEED(w3, p + "ffn.3.weight", D, 512); NEED(b3, p + "ffn.3.bias", D);
            // per-op path
            TRY(upload_packed(prec, wo->data.data(), (size_t)D * D, bw.out, (size_t)i * D * D));
            TRY(up_f32(bw.b_out + (size_t)i * D, bo->data.data(), D));
            TRY(upload_packed(prec, w0->data.data(), (size_t)512 * 512, bw.f1, (size_t)i * 512 * 512));
            TRY(up_f32(bw.b_f1 + (size_t)i * 512, b0->data.data(), 512));
            TRY(up_f32(bw.ln_g + (size_t)i * 512, g->data.data(), 512));
            TRY(up_f32(bw.ln_b + (size_t)i * 512, be->data.data(), 512));
            TRY(upload_packed(prec, w3->data.data(), (size_t)D * 512, bw.f2, (size_t)i * D * 512));
            TRY(up_f32(bw.b_f2 + (size_t)i * D, b3->data.data(), D));
            // fused tail: Wcat = [W1x | W1m Wo], bcat = b1 + W1m bo (double precision fold)
            std::vector<double> cat((size_t)512 * 512), w2d(w3->data.begin(), w3->data.end());
            std::vector<float> bc(512);
            for (int n = 0; n < 512; ++n) {
                const float* w1row = &w0->data[(size_t)n * 512];
                for (int k = 0; k < 256; ++k) cat[(size_t)n * 512 + k] = w1row[k];
                double bacc = b0->data[n];
                for (int j = 0; j < 256; ++j) bacc += (double)w1row[256 + j] * (double)bo->data[j];
                bc[n] = (float)bacc;
                for (int k = 0; k < 256; ++k) {
                    double acc = 0.0;
                    for (int j = 0; j < 256; ++j) acc += (double)w1row[256 + j] * (double)wo->data[(size_t)j * 256 + k];
                    cat[(size_t)n * 512 + 256 + k] = acc;
                }
            }
            TRY(upload_fragment_packed(prec, cat, 512, 512, bw.tail_cat + (size_t)i * e->tail_cat_layer_bytes));
            TRY(upload_fragment_packed(prec, w2d, 256, 512, bw.tail_2 + (size_t)i * e->tail_2_layer_bytes));
            TRY(up_f32(bw.b_cat + (size_t)i * 512, bc.data(), 512));
        }
        {   // cross: [to_qk ; to_v] share one GEMM (both applied to both images, ref :204-205)
            NEED(wq, c + "to_qk.weight", D, D); NEED(bq, c + "to_qk.bias", D);
            NEED(wv, c + "to_v.weight", D, D); NEED(bv, c + "to_v.bias", D);
            std::vector<float> pw((size_t)512 * D), pb(512);
            std::memcpy(pw.data(), wq->data.data(), (size_t)D * D * 4);
            std::memcpy(pw.data() + (size_t)D * D, wv->data.data(), (size_t)D * D * 4);
            std::memcpy(pb.data(), bq->data.data(), D * 4); std::memcpy(pb.data() + D, bv->data.data(), D * 4);
            TRY(upload_fragment_packed(prec, proj_row_permutation(pw, 512, cb.n_qk_groups, D), 512, D, cb.qkv_p + (size_t)i * cb.qkv_layer_bytes));
            TRY(up_f32(cb.b_qkv + (size_t)i * 512, pb.data(), 512));
        }
        {
            const std::string a = "log_assignment." + std::to_string(i) + ".";
            NEED(wf, a + "final_proj.weight", D, D); NEED(bf, a + "final_proj.bias", D);
            NEED(wm, a + "matchability.weight", 1, D); NEED(bm, a + "matchability.bias", 1);
            TRY(upload_fragment_packed(prec, std::vector<double>(wf->data.begin(), wf->data.end()), D, D, e->w_final_p + (size_t)i * e->final_layer_bytes));
            TRY(up_f32(e->b_final + (size_t)i * D, bf->data.data(), D));
            TRY(up_f32(e->w_match + (size_t)i * D, wm->data.data(), D));
            TRY(up_f32(e->b_match + i, bm->data.data(), 1));
        }
        if (i < L - 1) {
            const std::string tkn = "token_confidence." + std::to_string(i) + ".token.0.";
            NEED(wt, tkn + "weight", 1, D); NEED(bt, tkn + "bias", 1);
            TRY(up_f32(e->w_tok + (size_t)i * D, wt->data.data(), D));
            TRY(up_f32(e->b_tok + i, bt->data.data(), 1));
        }
    }
#undef NEED
    e->weights_ready = true;
    return LG_OK;
}

}  // extern "C"
