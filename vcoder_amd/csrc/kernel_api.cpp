// kernel_api.cpp — C-ABI entry points over the individual kernel launchers (declared in
// include/vcoder_kernels.h).  The `-m gpu` parity tests call every kernel through these with device
// pointers; the CPU emulator build (tests/emu) exports the same symbols over host pointers.
#include <stdexcept>

#include "kernels.h"
using namespace vc;

#define VCK_EXPORT extern "C" __attribute__((visibility("default")))
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

VCK_EXPORT void vck_gemm(const uint16_t* A, const uint16_t* W, const float* bias, void* out, int M, int N, int K,
                         int lda, int ldw, int ldo, int epi, void* stream) {
    GemmArgs a{A, W, bias, out, M, N, K, lda, ldw, ldo};
    launch_gemm(a, epi, S(stream));
}
VCK_EXPORT void vck_gemm_ws(const uint16_t* A, const uint16_t* W, const float* bias, void* out, int M, int N, int K,
                            int lda, int ldw, int ldo, int epi, float* ws, size_t ws_bytes, void* stream) {
    GemmArgs a{A, W, bias, out, M, N, K, lda, ldw, ldo};
    a.ws = ws;
    a.ws_bytes = ws_bytes;
    launch_gemm(a, epi, S(stream));
}
VCK_EXPORT void vck_gemm_f8(const uint8_t* A, const float* a_scale, const uint8_t* W, const float* w_scale, void* out, int M,
                            int N, int K, int ldo, int epi, float* ws, size_t ws_bytes, void* stream) {
    GemmArgs a{reinterpret_cast<const bf16_t*>(A), reinterpret_cast<const bf16_t*>(W), nullptr, out, M, N, K, K, K, ldo};
    a.ws = ws;
    a.ws_bytes = ws_bytes;
    a.f8 = 1;
    a.a_scale = a_scale;
    a.w_scale = w_scale;
    launch_gemm(a, epi, S(stream));
}
/* the QKV GEMM of a prefill layer with RoPE + head split + KV write in its epilogue (EPI_QKV; kernels.h QkvEpiArgs): A [B * T, lda]
 * bf16 (or e4m3 rows + a_scale with f8 != 0: W then e4m3 [3 D, K] + w_scale), W [3 D, K]; hd = 128 */
VCK_EXPORT void vck_gemm_qkv(const void* A, const float* a_scale, const void* W, const float* w_scale, const float* bias, int B, int T,
                             int H, int K, int lda, uint16_t* q, uint16_t* k, uint16_t* v, uint16_t* vt, uint8_t* k8, uint8_t* v8,
                             int q_stride, int kv_stride, int vt_stride, int kv8_stride, const float* rope_cos, const float* rope_sin,
                             int f8, float* ws, size_t ws_bytes, void* stream) {
    const int Tp = (T + 31) / 32 * 32;
    GemmArgs a{reinterpret_cast<const bf16_t*>(A), reinterpret_cast<const bf16_t*>(W), bias, nullptr, B * Tp, 3 * H * 128, K, lda, K, 0};
    a.ws = ws;
    a.ws_bytes = ws_bytes;
    a.f8 = f8;
    a.a_scale = a_scale;
    a.w_scale = w_scale;
    a.qe = QkvEpiArgs{q, k, v, vt, k8, v8, rope_cos, rope_sin, B, T, Tp, H, q_stride, kv_stride, vt_stride, kv8_stride};
    launch_gemm(a, EPI_QKV, S(stream));
}
VCK_EXPORT void vck_quant_act_rows(const uint16_t* A, int lda, uint8_t* Q, float* scale, int M, int K, void* stream) {
    launch_quant_act_rows(A, lda, Q, scale, M, K, S(stream));
}
VCK_EXPORT void vck_gemv(const uint16_t* X, const uint16_t* Wp, void* out, int M, int N, int K, int ldo, int epi,
                         void* stream) {
    GemvArgs a{};
    a.X = X; a.Wp = Wp; a.out = out; a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    launch_gemv(a, epi, S(stream));
}
VCK_EXPORT void vck_gemv_ex(const uint16_t* X, const void* Wp, const float* wscale, void* out, const float* ssq_in,
                            float* ssq_out, const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch,
                            unsigned* sk_counters, int ksplit, int M, int N, int K, int ldo, int epi, void* stream) {
    GemvArgs a{};
    a.X = X; a.Wp = reinterpret_cast<const uint16_t*>(Wp); a.wscale = wscale; a.out = out; a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    a.ssq_in = ssq_in; a.ssq_out = ssq_out; a.xg_w = xg_w; a.xg_out = xg_out; a.npart = npart; a.eps = eps;
    a.sk_scratch = sk_scratch; a.sk_counters = sk_counters; a.ksplit = ksplit;
    launch_gemv(a, epi, S(stream));
}
VCK_EXPORT void vck_attention_decode_fused(const uint16_t* qkv, uint16_t* k, uint16_t* v, uint16_t* out, int B, int H,
                                           int hd, int kv_stride, const int* pos_dev, const float* rope_cos,
                                           const float* rope_sin, float scale, void* stream) {
    AttnDecodeFusedArgs a{qkv, k, v, out, B, H, hd, kv_stride, pos_dev, rope_cos, rope_sin, scale, 0, nullptr};
    launch_attention_decode_fused(a, S(stream));
}
VCK_EXPORT void vck_attention_decode_rows(const uint16_t* qkv, uint16_t* k, uint16_t* v, uint16_t* out, int B, int H, int hd,
                                          int kv_stride, const int* pos_rows, int pos_stride, const int* active_rows,
                                          const float* rope_cos, const float* rope_sin, float scale, void* stream) {
    AttnDecodeFusedArgs a{qkv, k, v, out, B, H, hd, kv_stride, pos_rows, rope_cos, rope_sin, scale, pos_stride, active_rows};
    launch_attention_decode_fused(a, S(stream));
}
VCK_EXPORT int vck_attention_verify(const uint16_t* qkv, void* k, void* v, uint16_t* out, int B, int H, int hd, int kv_stride, int Q,
                                    const int* pos_rows, int pos_stride, const int* nq, const float* rope_cos, const float* rope_sin,
                                    float scale, int kv8, const uint8_t* key_mask, int mask_stride, void* stream) {
    if (Q < 1 || Q > 8 || (hd != 128 && hd != 64) || attention_verify_lds_bytes(Q, hd, kv8, kv_stride) > ATTN_VERIFY_LDS_MAX) return -1;
    AttnVerifyArgs a{qkv, k, v, out, B, H, hd, kv_stride, Q, pos_rows, pos_stride, nq, rope_cos, rope_sin, scale, kv8, key_mask, mask_stride};
    launch_attention_verify(a, S(stream));
    return 0;
}
VCK_EXPORT int vck_attention_fanout(const uint16_t* qkv, void* k, void* v, uint16_t* out, int G, int H, int hd, int kv_stride, int n,
                                    int cache_rows, const int* pos_rows, int pos_stride, const int* prefix_len, const int* prefix_row,
                                    const float* rope_cos, const float* rope_sin, float scale, int kv8, void* stream) {
    if (n < 1 || n > 8 || (hd != 128 && hd != 64) || attention_fanout_lds_bytes(n, hd, kv8, kv_stride) > ATTN_VERIFY_LDS_MAX) return -1;
    AttnFanoutArgs a{qkv, k, v, out, G, H, hd, kv_stride, n, cache_rows, pos_rows, pos_stride, prefix_len, prefix_row, rope_cos, rope_sin,
                     scale, kv8};
    launch_attention_fanout(a, S(stream));
    return 0;
}
VCK_EXPORT void vck_select_embed(const float* logits, int ldl, int* rows, int* next_tok, int* out_ids, const uint16_t* embed,
                                 float* x, float* ssq, const float* xg_w, uint16_t* xg, int D, int npart, int V, int nrows,
                                 int advance, void* stream) {
    SelectArgs a{logits, ldl, rows, next_tok, out_ids, embed, x, ssq, xg_w, xg, D, npart, V, nrows, advance, 0, 0};
    launch_select_embed(a, S(stream));
}
VCK_EXPORT void vck_spec_draft(const int* rows, const int* out_ids, const int* lookup, const int* lookup_len, int lookup_stride,
                               const int* prompt, const int* prompt_len, int prompt_stride, int* tok, int* nq, int B, int Q, int k,
                               int max_ngram, int V, void* stream) {
    SpecDraftArgs a{rows, out_ids, lookup, lookup_len, lookup_stride, prompt, prompt_len, prompt_stride, tok, nq, B, Q, k, max_ngram, V};
    launch_spec_draft(a, S(stream));
}
VCK_EXPORT void vck_spec_accept(const float* logits, int ldl, int V, int* rows, int* next_tok, int* out_ids, const int* tok, const int* nq,
                                int B, int Q, int* counters, const float* scratch_lp, const int* scratch_ids, int scratch_k, float* lp_tok,
                                float* lp_top, int* lp_ids, int lp_k, void* stream) {
    SpecAcceptArgs a{logits, ldl, V, rows, next_tok, out_ids, tok, nq, B, Q, counters, scratch_lp, scratch_ids, scratch_k, lp_tok, lp_top,
                     lp_ids, lp_k};
    launch_spec_accept(a, S(stream));
}
VCK_EXPORT void vck_spec_accept_sel(const float* logits, int ldl, int V, int* rows, int* next_tok, int* out_ids, const int* tok, const int* nq,
                                    int B, int Q, int* counters, const float* scratch_lp, const int* scratch_ids, int scratch_k, float* lp_tok,
                                    float* lp_top, int* lp_ids, int lp_k, const int* sel, const float* scratch_chosen, void* stream) {
    SpecAcceptArgs a{logits, ldl, V, rows, next_tok, out_ids, tok, nq, B, Q, counters, scratch_lp, scratch_ids, scratch_k, lp_tok, lp_top,
                     lp_ids, lp_k, sel, scratch_chosen};
    launch_spec_accept(a, S(stream));
}
VCK_EXPORT void vck_spec_select(const float* logits, int ldl, int V, const int* rows, const int* nq, int* sel, int B, int Q, int lds_floats,
                                void* stream) {
    SpecSelectArgs a{logits, ldl, V, rows, nq, sel, B, Q, 0};
    launch_spec_select(a, lds_floats, S(stream));
}
VCK_EXPORT void vck_warp_support(const float* logits, int ldl, int V, const int* rows, int nrows, int* keep, int lds_floats, void* stream) {
    launch_warp_support(logits, ldl, V, rows, nrows, keep, lds_floats, S(stream));
}
VCK_EXPORT int vck_row_state_stride() { return RS_STRIDE; }
VCK_EXPORT void vck_uniform_probe(const uint32_t* h, float* u, float* gumbel, int n, void* stream) {
    launch_uniform_probe(h, u, gumbel, n, S(stream));
}
VCK_EXPORT void vck_token_logprob(const float* logits, int ldl, const int* target, float* logprob, int rows, int V, void* stream) {
    launch_token_logprob(logits, ldl, target, logprob, rows, V, S(stream));
}
VCK_EXPORT void vck_topk_logprob(const float* logits, int ldl, const int* chosen, float* chosen_lp, float* top_lp, int* top_ids,
                                 int rows, int V, int K, int lds_floats, void* stream) {
    if (K < 0 || K > VC_MAX_TOP_LOGPROBS) return;   // nothing is launched, nothing written
    TopkLogprobArgs a{logits, ldl, chosen, chosen_lp, top_lp, top_ids, V, K, nullptr, nullptr, 0};
    launch_topk_logprob(a, rows, lds_floats, S(stream));
}
VCK_EXPORT void vck_beam_step(const float* cand_lp, const int* cand_id, float* beam_score, int* rows, int* next_tok, int* perm,
                              int* tok_tab, int* parent_tab, int* seq, int* hyp, const float* hyp_den, const float* done_den,
                              const int* params, int* flags, int B, int n, int advance, void* stream) {
    BeamStepArgs a{cand_lp, cand_id, beam_score, rows, next_tok, perm, tok_tab, parent_tab, seq, hyp, hyp_den, done_den, params, flags,
                   B, n, advance};
    launch_beam_step(a, S(stream));
}
VCK_EXPORT void vck_kv_permute_tail(void* kcache, void* vcache, void* tmp, const int* perm, const int* start, const int* rows, int R,
                                    int H, int cap_positions, int pos_bytes, int span_positions, void* stream) {
    launch_kv_permute_tail(kcache, vcache, tmp, perm, start, rows, R, H, (size_t)cap_positions * pos_bytes, pos_bytes,
                           (size_t)span_positions * pos_bytes, S(stream));
}
VCK_EXPORT void vck_logits_process(const float* logits, int ldl, float* out, int ldo, const int* rows, const int* prompt_ids,
                                   const int* out_ids, const int* bad_words, int nrows, int V, void* stream) {
    LogitsProcessArgs a{logits, ldl, out, ldo, const_cast<int*>(rows), prompt_ids, out_ids, bad_words, V};   // (no tables: read only)
    launch_logits_process(a, nrows, S(stream));
}
VCK_EXPORT void vck_logits_process_constrained(const float* logits, int ldl, float* out, int ldo, int* rows, const int* prompt_ids,
                                               const int* out_ids, const int* bad_words, const int* state_off, const int* edge_tok,
                                               const int* edge_next, const int* default_next, int n_states, int nrows, int V,
                                               void* stream) {
    LogitsProcessArgs a{logits, ldl, out, ldo, rows, prompt_ids, out_ids, bad_words, V};
    if (state_off && edge_tok && edge_next && default_next && n_states > 0) {
        a.cn_state_off = state_off;
        a.cn_edge_tok = edge_tok;
        a.cn_edge_next = edge_next;
        a.cn_default_next = default_next;
        a.cn_states = n_states;
    }
    launch_logits_process(a, nrows, S(stream));
}
VCK_EXPORT void vck_logits_process_verify(const float* logits, int ldl, float* out, int ldo, const int* rows, const int* prompt_ids,
                                          const int* out_ids, const int* bad_words, const int* tok, const int* nq, int B, int Q, int V,
                                          void* stream) {
    if (B < 1 || Q < 1) return;   // nothing is launched, nothing written
    LogitsProcessArgs a{logits, ldl, out, ldo, const_cast<int*>(rows), prompt_ids, out_ids, bad_words, V, Q, tok, nq};
    launch_logits_process(a, B * Q, S(stream));
}
VCK_EXPORT void vck_guidance_combine(const float* cond, const float* uncond, int ldl, float* out, int ldo, const int* rows,
                                     float* scalars, int nrows, int V, void* stream) {
    GuidanceCombineArgs a{cond, uncond, ldl, out, ldo, rows, scalars, V};
    launch_guidance_combine(a, nrows, S(stream));
}
VCK_EXPORT void vck_guidance_follow(int* rows, int* next_tok, float* x, float* ssq, uint16_t* xg, int B, int D, int npart, int advance,
                                    void* stream) {
    if (B < 1 || D < 8 || D % 8 != 0) return;   // nothing is launched, nothing written
    GuidanceFollowArgs a{rows, next_tok, x, ssq, reinterpret_cast<bf16_t*>(xg), B, D, npart, advance};
    launch_guidance_follow(a, S(stream));
}
VCK_EXPORT void vck_embed_tokens_ssq(const int* tok, const uint16_t* embed, float* x, float* ssq, const float* xg_w,
                                     uint16_t* xg, int B, int D, int npart, void* stream) {
    launch_embed_tokens_ssq(tok, embed, x, ssq, xg_w, xg, B, D, npart, S(stream));
}
VCK_EXPORT void vck_quantize_fp8(uint16_t* W, uint8_t* Wq, float* scale, int N, int K, void* stream) {
    launch_quantize_fp8(W, Wq, scale, N, K, S(stream));
}
VCK_EXPORT void vck_quantize_fp8_rows(uint16_t* W, uint8_t* Wq, float* scale, uint8_t* Wrow, int N, int K, void* stream) {
    launch_quantize_fp8(W, Wq, scale, N, K, S(stream), Wrow);
}
VCK_EXPORT void vck_pack_weight(const uint16_t* W, uint16_t* Wp, int N, int K, void* stream) {
    launch_pack_weight(W, Wp, N, K, S(stream));
}
VCK_EXPORT void vck_interleave_rows(const uint16_t* g, const uint16_t* u, uint16_t* out, int F, int K, void* stream) {
    launch_interleave_rows(g, u, out, F, K, S(stream));
}
VCK_EXPORT void vck_layernorm(const float* x, const float* w, const float* b, uint16_t* y, int rows, int D, float eps,
                              void* stream) {
    launch_layernorm(x, w, b, y, rows, D, eps, S(stream));
}
VCK_EXPORT void vck_rmsnorm(const float* x, const int* row_idx, const float* w, uint16_t* y, int rows, int D, float eps,
                            void* stream) {
    if (row_idx) launch_rmsnorm_rows(x, row_idx, w, y, rows, D, eps, S(stream));
    else launch_rmsnorm(x, w, y, rows, D, eps, S(stream));
}
VCK_EXPORT void vck_rmsnorm_ld(const float* x, const float* w, uint16_t* y, int rows, int D, float eps, int ldy, void* stream) {
    launch_rmsnorm(x, w, y, rows, D, eps, S(stream), ldy);
}
VCK_EXPORT void vck_rmsnorm_q8(const float* x, const float* w, uint8_t* q, float* scale, int rows, int D, float eps, void* stream) {
    launch_rmsnorm_q8(x, w, q, scale, rows, D, eps, S(stream));
}
VCK_EXPORT void vck_im2col(const float* pixels, uint16_t* cols, int n_img, int image, int patch, int Kpad, void* stream) {
    launch_im2col(pixels, cols, n_img, image, patch, Kpad, S(stream));
}
VCK_EXPORT void vck_vit_embed_ln(const float* patches, const float* cls, const float* pos, const float* w,
                                 const float* b, float* x, int n_img, int T, int D, float eps, void* stream) {
    launch_vit_embed_ln(patches, cls, pos, w, b, x, n_img, T, D, eps, S(stream));
}
VCK_EXPORT void vck_select_rows_bf16(const float* x, uint16_t* y, int n_img, int T, int skip, int D, void* stream) {
    launch_select_rows_bf16(x, y, n_img, T, skip, D, S(stream));
}
VCK_EXPORT void vck_qkv_split(const uint16_t* qkv, uint16_t* q, uint16_t* k, uint16_t* vt, int B, int T, int H, int hd,
                              int q_stride, int kv_stride, const int* pos0_dev, const float* rope_cos,
                              const float* rope_sin, void* stream) {
    QkvSplitArgs a{qkv, q, k, vt, B, T, H, hd, q_stride, kv_stride, nullptr, rope_cos, rope_sin, nullptr, 0};
    (void)pos0_dev;
    launch_qkv_split(a, S(stream));
}
VCK_EXPORT void vck_qkv_split_kv(const uint16_t* qkv, uint16_t* q, uint16_t* k, uint16_t* v, uint16_t* vt, int B, int T, int H,
                                 int hd, int q_stride, int kv_stride, int vt_stride, const float* rope_cos,
                                 const float* rope_sin, void* stream) {
    QkvSplitArgs a{qkv, q, k, vt, B, T, H, hd, q_stride, kv_stride, nullptr, rope_cos, rope_sin, v, vt_stride};
    launch_qkv_split(a, S(stream));
}
/* the prefill's split + RoPE writing an e4m3 KV cache (k8 / v8 [B,H,kv8_stride,hd] bytes; the fp8 weight format): K bf16 rows go
 * to the per-call scratch `k` (stride kv_stride) the flash kernel reads */
VCK_EXPORT void vck_qkv_split_kv8(const uint16_t* qkv, uint16_t* q, uint16_t* k, uint8_t* k8, uint8_t* v8, uint16_t* vt, int B, int T,
                                  int H, int hd, int q_stride, int kv_stride, int vt_stride, int kv8_stride, const float* rope_cos,
                                  const float* rope_sin, void* stream) {
    QkvSplitArgs a{qkv, q, k, vt, B, T, H, hd, q_stride, kv_stride, nullptr, rope_cos, rope_sin, nullptr, vt_stride, k8, v8, kv8_stride};
    launch_qkv_split(a, S(stream));
}
/* the fused decode attention of the bf16 step over e4m3 caches */
VCK_EXPORT void vck_attention_decode_kv8(const uint16_t* qkv, uint8_t* k, uint8_t* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                                         const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                                         const float* rope_sin, float scale, void* stream) {
    AttnDecodeFusedArgs a{qkv, reinterpret_cast<uint16_t*>(k), reinterpret_cast<uint16_t*>(v), out, B, H, hd, kv_stride, pos_rows,
                          rope_cos, rope_sin, scale, pos_stride, active_rows, 3};
    launch_attention_decode_fused(a, S(stream));
}
VCK_EXPORT void vck_attention(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* out, int B, int H,
                              int T, int hd, int q_stride, int kv_stride, int causal, float scale, void* stream) {
    AttnArgs a{q, k, vt, out, B, H, T, hd, q_stride, kv_stride, causal, scale};
    launch_attention(a, S(stream));
}
/* extend attention: n queries per (b, h) at positions P .. P+n-1 over the P+n keys of a key-major decode cache (bf16, or e4m3
 * when kv8); key_mask [B][mask_stride] bytes (0 = hidden) or NULL */
VCK_EXPORT void vck_attention_extend(const uint16_t* q, const void* k, const void* v, uint16_t* out, int B, int H, int n, int P,
                                     int hd, int q_stride, int kv_stride, int kv8, float scale, const uint8_t* key_mask,
                                     int mask_stride, void* stream) {
    AttnExtendArgs a{q, k, v, out, B, H, n, P, hd, q_stride, kv_stride, kv8, scale, key_mask, mask_stride};
    launch_attention_extend(a, S(stream));
}
VCK_EXPORT void vck_splice(const int* row_src, int nrows, const uint16_t* embed, const uint16_t* feats, float* x, int D,
                           void* stream) {
    launch_splice(row_src, nrows, embed, feats, x, D, S(stream));
}
VCK_EXPORT void vck_embed_tokens(const int* tok, const uint16_t* embed, float* x, int B, int D, void* stream) {
    launch_embed_tokens(tok, embed, x, B, D, S(stream));
}
VCK_EXPORT void vck_greedy(const float* logits, int* next_tok, int* out_ids, int* finished, int* step_dev, int B, int V,
                           int max_new, int eos_id, int pad_id, void* stream) {
    GreedyArgs a{logits, next_tok, out_ids, finished, step_dev, B, V, max_new, eos_id, pad_id};
    launch_greedy(a, S(stream));
}
VCK_EXPORT void vck_advance(int* step_dev, int* pos_dev, int* ctx_dev, void* stream) {
    launch_advance(step_dev, pos_dev, ctx_dev, S(stream));
}
VCK_EXPORT void vck_synth_bf16(uint16_t* out, uint64_t n, uint32_t tseed, float offset, float halfwidth, void* stream) {
    launch_synth_bf16(out, (size_t)n, tseed, offset, halfwidth, S(stream));
}
VCK_EXPORT void vck_synth_f32_rounded(float* out, uint64_t n, uint32_t tseed, float offset, float halfwidth, int rounding, void* stream) {
    launch_synth_f32_rounded(out, (size_t)n, tseed, offset, halfwidth, rounding, S(stream));
}
VCK_EXPORT void vck_synth_f32(float* out, uint64_t n, uint32_t tseed, float offset, float halfwidth, void* stream) {
    launch_synth_f32(out, (size_t)n, tseed, offset, halfwidth, S(stream));
}
VCK_EXPORT void vck_f32_to_bf16(const float* in, uint16_t* out, uint64_t n, void* stream) {
    launch_f32_to_bf16(in, out, (size_t)n, S(stream));
}
VCK_EXPORT void vck_bf16_to_f32(const uint16_t* in, float* out, uint64_t n, void* stream) {
    launch_bf16_to_f32(in, out, (size_t)n, S(stream));
}

// ---- strict (fp32) kernels -----------------------------------------------------------------------------------------
VCK_EXPORT void vck_gemm_f32(const float* A, const uint16_t* W, const float* bias, float* out, int M, int N, int K, int lda,
                             int ldw, int ldo, int epi, void* stream) {
    GemmF32Args a{A, W, bias, out, M, N, K, lda, ldw, ldo};
    launch_gemm_f32(a, epi, S(stream));
}
/* ... with the lo plane of an inexact checkpoint's weight: w = W + W_lo */
VCK_EXPORT void vck_gemm_f32_wlo(const float* A, const uint16_t* W, const uint16_t* W_lo, const float* bias, float* out, int M, int N,
                                 int K, int lda, int ldw, int ldo, int epi, void* stream) {
    GemmF32Args a{A, W, bias, out, M, N, K, lda, ldw, ldo};
    a.W_lo = W_lo;
    launch_gemm_f32(a, epi, S(stream));
}
VCK_EXPORT void vck_f32_to_bf16_planes(const float* in, uint16_t* hi, uint16_t* lo, uint64_t n, unsigned* inexact, void* stream) {
    launch_f32_to_bf16_planes(in, hi, lo, (size_t)n, inexact, S(stream));
}
VCK_EXPORT void vck_attention_f32(const float* q, const float* k, const float* v, float* out, int B, int H, int Tq, int hd,
                                  int q_stride, int kv_stride, int causal, int Tk, const int* pos0_dev, float scale,
                                  void* stream) {
    AttnF32Args a{q, k, v, out, B, H, Tq, hd, q_stride, kv_stride, causal, Tk, pos0_dev, scale};
    launch_attention_f32(a, S(stream));
}
VCK_EXPORT void vck_qkv_rope_f32(const float* qkv, float* q, float* k, float* v, int B, int T, int H, int hd, int q_stride,
                                 int kv_stride, const int* pos0_dev, const float* rope_cos, const float* rope_sin,
                                 void* stream) {
    QkvF32Args a{qkv, q, k, v, B, T, H, hd, q_stride, kv_stride, pos0_dev, rope_cos, rope_sin};
    launch_qkv_rope_f32(a, S(stream));
}

// ---- precision mode "split" (DESIGN.md section 5b): every MFMA operand as bf16 hi + lo -------------------------------------
VCK_EXPORT void vck_gemm_split(const uint16_t* A, const uint16_t* W, const float* bias, void* out, int M, int N, int Kw, int lda,
                               int ldo, int epi, int split_out, float* ws, size_t ws_bytes, void* stream) {
    GemmArgs a{A, W, bias, out, M, N, 2 * Kw, lda, Kw, ldo};
    a.kwrap = Kw / 64;
    a.split_out = split_out;
    a.ws = ws;
    a.ws_bytes = ws_bytes;
    launch_gemm(a, epi, S(stream));
}
VCK_EXPORT void vck_gemv_split(const uint16_t* X, const void* Wp, const float* wscale, void* out, const float* ssq_in,
                               float* ssq_out, const float* xg_w, uint16_t* xg_out, int npart, float eps, int M, int N, int K,
                               int ldo, int epi, int G, void* stream) {
    GemvArgs a{};
    a.X = X; a.Wp = reinterpret_cast<const uint16_t*>(Wp); a.wscale = wscale; a.out = out; a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    a.ssq_in = ssq_in; a.ssq_out = ssq_out; a.xg_w = xg_w; a.xg_out = xg_out; a.npart = npart; a.eps = eps;
    a.split_rows = G;
    launch_gemv(a, epi, S(stream));
}
/* ... with the lo plane of an inexact checkpoint's weight ([N, Kw] like W): a third K segment a_hi . w_lo (K = 3 Kw) */
VCK_EXPORT void vck_gemm_split_wlo(const uint16_t* A, const uint16_t* W, const uint16_t* W_lo, const float* bias, void* out, int M,
                                   int N, int Kw, int lda, int ldo, int epi, int split_out, float* ws, size_t ws_bytes, void* stream) {
    GemmArgs a{A, W, bias, out, M, N, (W_lo ? 3 : 2) * Kw, lda, Kw, ldo};
    a.kwrap = Kw / 64;
    a.split_out = split_out;
    if (W_lo) a.w_lo_off = (long long)(reinterpret_cast<const char*>(W_lo) - reinterpret_cast<const char*>(W));
    a.ws = ws;
    a.ws_bytes = ws_bytes;
    launch_gemm(a, epi, S(stream));
}
/* the split decode GEMV (G > 0) with the packed lo plane of an inexact checkpoint's weight */
VCK_EXPORT void vck_gemv_split_wlo(const uint16_t* X, const void* Wp, const void* Wp_lo, void* out, const float* ssq_in, float* ssq_out,
                                   const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch,
                                   unsigned long long sk_scratch_floats, unsigned* sk_counters, int sk_counters_n, int ksplit, int M,
                                   int N, int K, int ldo, int epi, int G, void* stream) {
    GemvArgs a{};
    a.X = X; a.Wp = reinterpret_cast<const uint16_t*>(Wp); a.Wp_lo = reinterpret_cast<const uint16_t*>(Wp_lo); a.out = out;
    a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    a.ssq_in = ssq_in; a.ssq_out = ssq_out; a.xg_w = xg_w; a.xg_out = xg_out; a.npart = npart; a.eps = eps;
    a.sk_scratch = sk_scratch; a.sk_counters = sk_counters; a.ksplit = ksplit;
    a.sk_scratch_floats = (size_t)sk_scratch_floats; a.sk_counters_n = sk_counters_n;
    a.split_rows = G;
    launch_gemv(a, epi, S(stream));
}
/* the decode GEMV with every argument (tests / tools): split rows G (0 = bf16 step), split-K buffers with their capacity */
VCK_EXPORT void vck_gemv_full(const uint16_t* X, const void* Wp, const float* wscale, void* out, const float* ssq_in,
                              float* ssq_out, const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch,
                              unsigned long long sk_scratch_floats, unsigned* sk_counters, int sk_counters_n, int ksplit, int M,
                              int N, int K, int ldo, int epi, int G, void* stream) {
    GemvArgs a{};
    a.X = X; a.Wp = reinterpret_cast<const uint16_t*>(Wp); a.wscale = wscale; a.out = out; a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    a.ssq_in = ssq_in; a.ssq_out = ssq_out; a.xg_w = xg_w; a.xg_out = xg_out; a.npart = npart; a.eps = eps;
    a.sk_scratch = sk_scratch; a.sk_counters = sk_counters; a.ksplit = ksplit;
    a.sk_scratch_floats = (size_t)sk_scratch_floats; a.sk_counters_n = sk_counters_n;
    a.split_rows = G;
    launch_gemv(a, epi, S(stream));
}
/* what vck_gemv_full would launch for these arguments under the current knobs, without launching (only which optional buffers are
 * present matters, not where they are): 0 and out = {form, waves, nt, r, xp, cl, fp8, wlo, ksplit, workgroups}, or -1 where the
 * call would be refused */
VCK_EXPORT int vck_gemv_plan(int M, int N, int K, int epi, int fp8, int split_rows, int ksplit, int has_sk,
                             unsigned long long sk_scratch_floats, int sk_counters_n, int has_wlo, int out[10]) {
    static float present_f;
    static unsigned present_u;
    static const uint16_t present_h = 0;
    GemvArgs a{};
    a.M = M; a.N = N; a.K = K; a.split_rows = split_rows; a.ksplit = ksplit;
    if (fp8) a.wscale = &present_f;
    if (has_sk) { a.sk_scratch = &present_f; a.sk_counters = &present_u; }
    a.sk_scratch_floats = (size_t)sk_scratch_floats; a.sk_counters_n = sk_counters_n;
    if (has_wlo) a.Wp_lo = &present_h;
    try {
        const GemvPlan p = gemv_plan(a, epi);
        const int per_wg = p.form == GEMV_FORM_WG ? p.waves * p.nt : p.nt;
        const int v[10] = {p.form, p.waves, p.nt, p.r, p.xp, p.cl, p.fp8, p.wlo, p.ksplit, (N / 16 + per_wg - 1) / per_wg * p.ksplit};
        for (int i = 0; i < 10; ++i) out[i] = v[i];
        return 0;
    } catch (const std::runtime_error&) {
        return -1;
    }
}
/* W4A16 (MXFP4): the load-time quantiser and the nibble-streaming decode GEMV (kernels.h GemvArgs::w4scale) */
VCK_EXPORT void vck_quantize_mxfp4(uint16_t* W, uint8_t* Wq, uint8_t* scale, int N, int K, void* stream) {
    launch_quantize_mxfp4(W, Wq, scale, N, K, S(stream));
}
static GemvArgs w4_args(const uint16_t* X, const void* Wq, const uint8_t* w4scale, void* out, const float* ssq_in, float* ssq_out,
                        const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch, unsigned* sk_counters, int ksplit,
                        int M, int N, int K, int ldo, int G) {
    GemvArgs a{};
    a.X = X; a.Wp = reinterpret_cast<const uint16_t*>(Wq); a.w4scale = w4scale; a.out = out; a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    a.ssq_in = ssq_in; a.ssq_out = ssq_out; a.xg_w = xg_w; a.xg_out = xg_out; a.npart = npart; a.eps = eps;
    a.sk_scratch = sk_scratch; a.sk_counters = sk_counters; a.ksplit = ksplit;
    a.split_rows = G;
    return a;
}
VCK_EXPORT void vck_gemv_w4(const uint16_t* X, const void* Wq, const uint8_t* w4scale, void* out, const float* ssq_in, float* ssq_out,
                            const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch, unsigned* sk_counters,
                            int ksplit, int M, int N, int K, int ldo, int epi, void* stream) {
    launch_gemv(w4_args(X, Wq, w4scale, out, ssq_in, ssq_out, xg_w, xg_out, npart, eps, sk_scratch, sk_counters, ksplit, M, N, K, ldo, 0), epi,
                S(stream));
}
VCK_EXPORT void vck_gemv_w4_split(const uint16_t* X, const void* Wq, const uint8_t* w4scale, void* out, const float* ssq_in,
                                  float* ssq_out, const float* xg_w, uint16_t* xg_out, int npart, float eps, int M, int N, int K, int ldo,
                                  int epi, int G, void* stream) {
    launch_gemv(w4_args(X, Wq, w4scale, out, ssq_in, ssq_out, xg_w, xg_out, npart, eps, nullptr, nullptr, 0, M, N, K, ldo, G), epi, S(stream));
}
/* what vck_gemv_w4 / vck_gemv_w4_split would launch: 0 and out = {form, waves, nt, r, xp, ksplit, workgroups}, or -1 where refused */
VCK_EXPORT int vck_gemv_w4_plan(int M, int N, int K, int epi, int split_rows, int ksplit, int has_sk, int out[7]) {
    static float present_f;
    static unsigned present_u;
    static const uint8_t present_b = 0;
    const GemvArgs a = w4_args(nullptr, nullptr, &present_b, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.f, has_sk ? &present_f : nullptr,
                               has_sk ? &present_u : nullptr, ksplit, M, N, K, N, split_rows);
    try {
        const GemvPlan p = gemv_plan(a, epi);
        const int v[7] = {p.form, p.waves, p.nt, p.r, p.xp, p.ksplit, (N / 16 + p.nt - 1) / p.nt * p.ksplit};
        for (int i = 0; i < 7; ++i) out[i] = v[i];
        return 0;
    } catch (const std::runtime_error&) {
        return -1;
    }
}
VCK_EXPORT void vck_set_gemv_w4_nt(int nt) { set_gemv_w4_nt(nt); }
/* split-mode GEMV: 0 = per-wave rings, 1 / -1 = workgroup-shared activation chunks (default) */
VCK_EXPORT void vck_set_gemv_variant(int v) { set_gemv_variant(v); }
VCK_EXPORT void vck_set_gemm_force_8phase(int on) { set_gemm_force_8phase(on != 0); }
VCK_EXPORT void vck_set_gemv_wide(int v) { set_gemv_wide(v); }
VCK_EXPORT unsigned long long vck_gemm_dma_launches() { return gemm_dma_launches(); }
VCK_EXPORT unsigned long long vck_gemm_8phase_launches() { return gemm_8phase_launches(); }
VCK_EXPORT unsigned long long vck_gemv_wide_launches() { return gemv_wide_launches(); }
VCK_EXPORT unsigned long long vck_gemv_wg_launches() { return gemv_wg_launches(); }
VCK_EXPORT void vck_rmsnorm_split(const float* x, const int* row_idx, const float* w, uint16_t* y, int rows, int D, float eps,
                                  int ldy, uint64_t lo_off, void* stream) {
    launch_rmsnorm_split(x, row_idx, w, y, rows, D, eps, ldy, (size_t)lo_off, S(stream));
}
VCK_EXPORT void vck_layernorm_split(const float* x, const float* w, const float* b, uint16_t* y, int rows, int D, float eps,
                                    int ldy, uint64_t lo_off, void* stream) {
    launch_layernorm_split(x, w, b, y, rows, D, eps, ldy, (size_t)lo_off, S(stream));
}
VCK_EXPORT void vck_qkv_split32(const float* qkv, uint16_t* q_hi, uint16_t* q_lo, uint16_t* k_hi, uint16_t* k_lo, uint16_t* vt_hi,
                                uint16_t* vt_lo, float* k32, float* v32, int B, int T, int H, int hd, int q_stride, int ks_stride,
                                int vt_stride, int kv_stride, const float* rope_cos, const float* rope_sin, void* stream) {
    QkvSplit32Args a{qkv, q_hi, q_lo, k_hi, k_lo, vt_hi, vt_lo, k32, v32, B, T, H, hd, q_stride, ks_stride, vt_stride, kv_stride,
                     rope_cos, rope_sin};
    launch_qkv_split32(a, S(stream));
}
/* the same with fp24 cache rows (k24 / v24: [B,H,kv_stride] x 3*hd bytes: hd x u16 | hd x u8) */
VCK_EXPORT void vck_qkv_split24(const float* qkv, uint16_t* q_hi, uint16_t* q_lo, uint16_t* k_hi, uint16_t* k_lo, uint16_t* vt_hi,
                                uint16_t* vt_lo, void* k24, void* v24, int B, int T, int H, int hd, int q_stride, int ks_stride,
                                int vt_stride, int kv_stride, const float* rope_cos, const float* rope_sin, void* stream) {
    QkvSplit32Args a{qkv, q_hi, q_lo, k_hi, k_lo, vt_hi, vt_lo, reinterpret_cast<float*>(k24), reinterpret_cast<float*>(v24), B, T, H, hd,
                     q_stride, ks_stride, vt_stride, kv_stride, rope_cos, rope_sin, 1};
    launch_qkv_split32(a, S(stream));
}
VCK_EXPORT void vck_attention_split(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                                    const uint16_t* vt_hi, const uint16_t* vt_lo, uint16_t* out, int B, int H, int T, int hd,
                                    int q_stride, int kv_stride, int causal, float scale, int ldo, int lo_off, void* stream) {
    AttnArgs a{q_hi, k_hi, vt_hi, out, B, H, T, hd, q_stride, kv_stride, causal, scale, 0, q_lo, k_lo, vt_lo, ldo, lo_off};
    launch_attention(a, S(stream));
}
VCK_EXPORT void vck_attention_decode_kv32(const float* qkv, float* k, float* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                                          const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                                          const float* rope_sin, float scale, int G, void* stream) {
    AttnDecodeFusedArgs a{reinterpret_cast<const uint16_t*>(qkv), reinterpret_cast<uint16_t*>(k), reinterpret_cast<uint16_t*>(v), out,
                          B, H, hd, kv_stride, pos_rows, rope_cos, rope_sin, scale, pos_stride, active_rows, 1, G};
    launch_attention_decode_fused(a, S(stream));
}
/* the same over fp24 caches */
VCK_EXPORT void vck_attention_decode_kv24(const float* qkv, void* k, void* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                                          const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                                          const float* rope_sin, float scale, int G, void* stream) {
    AttnDecodeFusedArgs a{reinterpret_cast<const uint16_t*>(qkv), reinterpret_cast<uint16_t*>(k), reinterpret_cast<uint16_t*>(v), out,
                          B, H, hd, kv_stride, pos_rows, rope_cos, rope_sin, scale, pos_stride, active_rows, 2, G};
    launch_attention_decode_fused(a, S(stream));
}

// ---- the attention kernels with the arguments the engine sets for a padded batch (key_mask / mask_stride) and for a prefill into a
// ---- cache (vt_stride): thin wrappers over the same argument structs (tests; include/vcoder_kernels.h)
VCK_EXPORT void vck_attention_ex(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* out, int B, int H, int T, int hd,
                                 int q_stride, int kv_stride, int vt_stride, int causal, float scale, const uint8_t* key_mask,
                                 int mask_stride, void* stream) {
    AttnArgs a{q, k, vt, out, B, H, T, hd, q_stride, kv_stride, causal, scale, vt_stride};
    a.key_mask = key_mask;
    a.mask_stride = mask_stride;
    launch_attention(a, S(stream));
}
VCK_EXPORT void vck_attention_split_ex(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                                       const uint16_t* vt_hi, const uint16_t* vt_lo, uint16_t* out, int B, int H, int T, int hd,
                                       int q_stride, int kv_stride, int vt_stride, int causal, float scale, int ldo, int lo_off,
                                       const uint8_t* key_mask, int mask_stride, void* stream) {
    AttnArgs a{q_hi, k_hi, vt_hi, out, B, H, T, hd, q_stride, kv_stride, causal, scale, vt_stride, q_lo, k_lo, vt_lo, ldo, lo_off};
    a.key_mask = key_mask;
    a.mask_stride = mask_stride;
    launch_attention(a, S(stream));
}
/* the fused decode attention, per-row form, over any cache format (kv_format: 0 bf16, 1 fp32, 2 fp24, 3 e4m3; G: the output row
 * groups of the fp32 / fp24 forms) with the rows' key masks */
VCK_EXPORT void vck_attention_decode_masked(const void* qkv, void* k, void* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                                            const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                                            const float* rope_sin, float scale, int kv_format, int G, const uint8_t* key_mask,
                                            int mask_stride, void* stream) {
    AttnDecodeFusedArgs a{reinterpret_cast<const uint16_t*>(qkv), reinterpret_cast<uint16_t*>(k), reinterpret_cast<uint16_t*>(v), out,
                          B, H, hd, kv_stride, pos_rows, rope_cos, rope_sin, scale, pos_stride, active_rows, kv_format, G, key_mask,
                          mask_stride};
    launch_attention_decode_fused(a, S(stream));
}
VCK_EXPORT void vck_attention_f32_masked(const float* q, const float* k, const float* v, float* out, int B, int H, int Tq, int hd,
                                         int q_stride, int kv_stride, int causal, int Tk, const int* pos0_dev, float scale,
                                         const uint8_t* key_mask, int mask_stride, void* stream) {
    AttnF32Args a{q, k, v, out, B, H, Tq, hd, q_stride, kv_stride, causal, Tk, pos0_dev, scale, key_mask, mask_stride};
    launch_attention_f32(a, S(stream));
}
/* output_attentions: q as fp32 (q32) or bf16 hi [+ lo]; k as fp32 (k32), bf16 hi [+ lo], e4m3 rows (k8) or fp24 rows (k24) */
VCK_EXPORT void vck_attn_probs(const float* q32, const uint16_t* q_hi, const uint16_t* q_lo, const float* k32, const uint16_t* k_hi,
                               const uint16_t* k_lo, const void* k24, const uint8_t* k8, float* out, int B, int H, int T, int hd,
                               int q_stride, int kv_stride, float scale, int Tk, int q_pos0, const uint8_t* key_mask,
                               int mask_stride, void* stream) {
    AttnProbsArgs a{};
    a.q32 = q32; a.q_hi = q_hi; a.q_lo = q_lo; a.k32 = k32; a.k_hi = k_hi; a.k_lo = k_lo; a.k24 = k24; a.k8 = k8; a.out = out;
    a.B = B; a.H = H; a.T = T; a.hd = hd; a.q_stride = q_stride; a.kv_stride = kv_stride; a.scale = scale;
    a.key_mask = key_mask; a.mask_stride = mask_stride; a.Tk = Tk; a.q_pos0 = q_pos0;
    launch_attn_probs(a, S(stream));
}
