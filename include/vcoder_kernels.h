/* vcoder_kernels.h — per-kernel C entry points of libvcoder_hip.so (unit-test / micro-benchmark surface).
 *
 * Every function enqueues ONE gfx950 kernel on `stream` (NULL = default stream) over DEVICE pointers; bf16 tensors
 * are raw uint16 bit patterns.  The `-m gpu` parity tests call each kernel through these at the true shapes of
 * VCoder-DS LLaVA-1.5-7b and compare with oracle/cpu_ref.py.  Each replaces a torch/HF op of the reference's hot
 * path; the file:line it restates is given per entry.
 */
#ifndef VCODER_KERNELS_H
#define VCODER_KERNELS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* nn.Linear / Conv2d-as-GEMM with fused epilogue: out = epi(A[M,K] . W[N,K]^T + bias).  epi: 0 bf16, 1 bf16 quick_gelu,
 * 2 bf16 erf-gelu, 3 fp32, 4 fp32 residual add in place, 5 SwiGLU over interleaved (gate,up) rows.
 * [HF] clip/modeling_clip.py:309-311,333,346-350; [HF] llama/modeling_llama.py:174-176,254-256,280;
 * vcoder_llava/model/multimodal_projector/builder.py:42-46 */
void vck_gemm(const uint16_t* A, const uint16_t* W, const float* bias, void* out, int M, int N, int K, int lda, int ldw,
              int ldo, int epi, void* stream);
/* same with an fp32 workspace (>= 64 MiB covers every shape): enables the deterministic split-K of a short last round of
 * 256x256 tiles (partials summed in k order by a fix-up launch) */
void vck_gemm_ws(const uint16_t* A, const uint16_t* W, const float* bias, void* out, int M, int N, int K, int lda, int ldw,
                 int ldo, int epi, float* ws, size_t ws_bytes, void* stream);
/* decode-time skinny GEMM (M<=16) over MFMA-fragment-packed weights.  epi: 0 bf16, 1 fp32, 2 fp32 residual, 3 SwiGLU */
void vck_gemv(const uint16_t* X, const uint16_t* Wp, void* out, int M, int N, int K, int ldo, int epi, void* stream);
/* general form.  RMSNorm ([HF] llama :53-70) is folded across producer and consumer instead of run as a pass:
 *   consumer  (ssq_in != NULL): X is xg = bf16(x * g) written by the producer and out = rstd[m] * (X @ W^T), with
 *             rstd[m] = rsqrt(sum_p ssq_in[m][p] / K + eps) from `npart` deterministic sum-of-squares partials;
 *   producer  (epi 2): ssq_out gets the partials of the updated residual rows and xg_out = bf16(residual * xg_w).
 * wscale != NULL: Wp holds W8A16 e4m3 bytes (vck_quantize_fp8) and wscale the per-output-row scales.
 * sk_scratch/sk_counters != NULL: deterministic split-K for matrices with few output tiles — `ksplit` workgroups per
 * tile (0 = let the launcher choose), partials [ksplit][N/16][2][256] fp32 summed in k order by the last arriver;
 * sk_counters [N/16][2] must be zero before the first launch (the kernel re-arms them).  M <= 32: rows 16..31 form a
 * second MFMA row group served by the same weight pass (the decode pool's steps). */
void vck_gemv_ex(const uint16_t* X, const void* Wp, const float* wscale, void* out, const float* ssq_in, float* ssq_out,
                 const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch, unsigned* sk_counters,
                 int ksplit, int M, int N, int K, int ldo, int epi, void* stream);
void vck_pack_weight(const uint16_t* W, uint16_t* Wp, int N, int K, void* stream);
/* W8A16 decode weights (BASELINE config C5): per-output-row power-of-two scale + OCP e4m3 bytes in the gemv's 64-wide
 * k super-tile order; W [N,K] bf16 is overwritten with the dequantised values (what the prefill GEMMs then read).
 * vck_gemv_ex streams the bytes. */
void vck_quantize_fp8(uint16_t* W, uint8_t* Wq, float* scale, int N, int K, void* stream);
/* the same, additionally leaving the bytes row-major in Wrow [N,K]: the weight operand of vck_gemm_f8 */
void vck_quantize_fp8_rows(uint16_t* W, uint8_t* Wq, float* scale, uint8_t* Wrow, int N, int K, void* stream);
/* W8A8 prefill GEMM (BASELINE config C5, "CDNA4 fp8 MFMA"): token rows of A [M,lda] bf16 -> e4m3 bytes Q [M,K] with a
 * per-row power-of-two scale (the rule of the weight rows); then
 *   out = epi( (Q @ Wrow^T) * a_scale[m] * w_scale[n] )
 * on v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales; twice the bf16 MFMA rate).  K % 128 == 0;
 * epi 0 bf16, 4 fp32 residual add, 5 SwiGLU.  ws: optional split-K workspace as for vck_gemm_ws. */
/* RMSNorm straight into that operand: the bytes / scales of vck_rmsnorm followed by vck_quant_act_rows, in one pass */
void vck_rmsnorm_q8(const float* x, const float* w, uint8_t* q, float* scale, int rows, int D, float eps, void* stream);
void vck_quant_act_rows(const uint16_t* A, int lda, uint8_t* Q, float* scale, int M, int K, void* stream);
void vck_gemm_f8(const uint8_t* A, const float* a_scale, const uint8_t* W, const float* w_scale, void* out, int M, int N,
                 int K, int ldo, int epi, float* ws, size_t ws_bytes, void* stream);
void vck_interleave_rows(const uint16_t* gate, const uint16_t* up, uint16_t* out, int F, int K, void* stream);
/* nn.LayerNorm ([HF] clip :370,379) and LlamaRMSNorm ([HF] llama :53-70); fp32 in, bf16 out */
void vck_layernorm(const float* x, const float* w, const float* b, uint16_t* y, int rows, int D, float eps, void* stream);
void vck_rmsnorm(const float* x, const int* row_idx, const float* w, uint16_t* y, int rows, int D, float eps, void* stream);
/* the same with a row stride: row r at y + r * ldy (elements; columns [D, ldy) are not written).  A prefill writes the bf16
 * operand rows of its QKV and gate / up GEMMs this way (ldy = D + 64 = their lda) */
void vck_rmsnorm_ld(const float* x, const float* w, uint16_t* y, int rows, int D, float eps, int ldy, void* stream);
/* CLIPVisionEmbeddings ([HF] clip :202-218): im2col of the k=s=14 conv; CLS + position + pre_layrnorm */
void vck_im2col(const float* pixels, uint16_t* cols, int n_img, int image, int patch, int Kpad, void* stream);
void vck_vit_embed_ln(const float* patches, const float* cls, const float* pos, const float* w, const float* b, float* x,
                      int n_img, int T, int D, float eps, void* stream);
/* feature_select (multimodal_encoder/clip_encoder.py:29-37) */
void vck_select_rows_bf16(const float* x, uint16_t* y, int n_img, int T, int skip, int D, void* stream);
/* head split + rotate_half RoPE ([HF] llama :113-160,259-262): qkv bf16 [B*T, 3*H*hd] -> Q [B,H,q_stride,hd],
 * K [B,H,kv_stride,hd], V^T [B,H,hd,kv_stride] (the MFMA A operand of the flash kernel's P.V).  pos0_dev is unused.
 * V^T is a scratch between this kernel and vck_attention and uses the flash kernel's KEY ORDER: inside every aligned block of 32
 * keys, position 8c + e (c = 0..3, e = 0..7) holds key 4c + (e & 3) + 16 (e >> 2) (csrc/attn.hip vt_chunk_key0) — the order in
 * which a lane's softmax numerators are packed into the P operand, so one 16-byte LDS read is a whole MFMA fragment.  A caller
 * that fills V^T itself (vck_attention's vt) must use the same order; strides are multiples of 64. */
void vck_qkv_split(const uint16_t* qkv, uint16_t* q, uint16_t* k, uint16_t* vt, int B, int T, int H, int hd, int q_stride,
                   int kv_stride, const int* pos0_dev, const float* rope_cos, const float* rope_sin, void* stream);
/* the LLM prefill form: K and V rows into the key-major KV cache (kv_stride keys per (b,h)) — what the decode steps stream —
 * and V^T into a per-call scratch of vt_stride columns for this layer's flash attention */
void vck_qkv_split_kv(const uint16_t* qkv, uint16_t* q, uint16_t* k, uint16_t* v, uint16_t* vt, int B, int T, int H, int hd,
                      int q_stride, int kv_stride, int vt_stride, const float* rope_cos, const float* rope_sin, void* stream);
/* softmax(QK^T*scale [+causal]) V, fp32 softmax ([HF] clip :259-277; [HF] llama eager_attention_forward :191-214) */
void vck_attention(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* out, int B, int H, int T, int hd,
                   int q_stride, int kv_stride, int causal, float scale, void* stream);
/* decode step, one launch per layer: RoPE of the new q/k + append of the K and V rows + attention over the cache.
 * K and V are both key-major [B,H,kv_stride,hd] (kv_stride <= 4096: a row's scores sit in LDS). */
void vck_attention_decode_fused(const uint16_t* qkv, uint16_t* k, uint16_t* v, uint16_t* out, int B, int H, int hd,
                                int kv_stride, const int* pos_dev, const float* rope_cos, const float* rope_sin, float scale,
                                void* stream);
/* the same with one position per row (row b reads pos_rows[b * pos_stride]; rows with active_rows[b * pos_stride] == 0 are
 * skipped): rows of different requests — different prompt lengths and step counts — share one decode step */
void vck_attention_decode_rows(const uint16_t* qkv, uint16_t* k, uint16_t* v, uint16_t* out, int B, int H, int hd,
                               int kv_stride, const int* pos_rows, int pos_stride, const int* active_rows,
                               const float* rope_cos, const float* rope_sin, float scale, void* stream);
/* verify attention (prompt-lookup speculation): nq[b] <= Q <= 8 consecutive query rows of sequence b — rows b * Q + j of qkv
 * [B * Q, 3 H hd] and out [B * Q, H hd] at positions pos_rows[b * pos_stride] + j — roped, appended to the cache (bf16, or e4m3
 * bytes when kv8) and attended in one launch over one read of the K and V streams.  Row j's output and the appended cache rows
 * are bit-identical to what vck_attention_decode_rows gives the row in a step of its own (an exactly-zero output may differ in
 * sign).  nq[b] <= 0 leaves sequence b untouched.  key_mask as above or NULL.  hd 128 or 64.  Returns 0, or -1 when the score
 * rows of Q queries over kv_stride keys do not fit the LDS of a CU (nothing is launched). */
int vck_attention_verify(const uint16_t* qkv, void* k, void* v, uint16_t* out, int B, int H, int hd, int kv_stride, int Q,
                         const int* pos_rows, int pos_stride, const int* nq, const float* rope_cos, const float* rope_sin,
                         float scale, int kv8, const uint8_t* key_mask, int mask_stride, void* stream);
/* fan-out attention (generate(num_return_sequences = n)): rows g n .. g n + n - 1 of qkv / out (G groups, n <= 8) continue one prompt
 * of prefix_len[g] keys held in positions [0, prefix_len[g]) of cache row prefix_row[g] (NULL: row g) of k / v
 * [cache_rows,H,kv_stride,hd]; row r appends at position pos_rows[g n * pos_stride] (>= the prefix length, one position per group)
 * of cache row r and reads its own keys behind the prefix from there.  A prefix key row is loaded once per (group, head).  Row r's
 * output and appended cache rows are bit-identical to what vck_attention_decode_rows gives it over a cache row that holds prefix +
 * own tail (an exactly-zero output may differ in sign).  hd 128 or 64.  Returns 0, or -1 when the score rows of n queries over
 * kv_stride keys do not fit the LDS of a CU (nothing is launched). */
int vck_attention_fanout(const uint16_t* qkv, void* k, void* v, uint16_t* out, int G, int H, int hd, int kv_stride, int n,
                         int cache_rows, const int* pos_rows, int pos_stride, const int* prefix_len, const int* prefix_row,
                         const float* rope_cos, const float* rope_sin, float scale, int kv8, void* stream);
/* extend attention (a multi-token continuation of a cached sequence): n roped queries per (b, h) (q [B,H,q_stride,hd]) at
 * positions P .. P+n-1 over keys [0, P+n) of the key-major decode cache (k, v [B,H,kv_stride,hd]: bf16, or e4m3 bytes when
 * kv8), causal inside the chunk; key_mask [B][mask_stride] bytes (0 = hidden; key 0 must be visible) or NULL.  hd 128.
 * out bf16 [B*n, H*hd], row b*n + t. */
void vck_attention_extend(const uint16_t* q, const void* k, const void* v, uint16_t* out, int B, int H, int n, int P, int hd,
                          int q_stride, int kv_stride, int kv8, float scale, const uint8_t* key_mask, int mask_stride,
                          void* stream);
/* embedding gather + feature splice (vcoder_ds_llava_arch.py:173-276,305) */
void vck_splice(const int* row_src, int nrows, const uint16_t* embed, const uint16_t* feats, float* x, int D, void* stream);
void vck_embed_tokens(const int* tok, const uint16_t* embed, float* x, int B, int D, void* stream);
/* greedy select with EOS/pad bookkeeping ([HF] generation/utils.py:2894,2925-2929) */
void vck_greedy(const float* logits, int* next_tok, int* out_ids, int* finished, int* step_dev, int B, int V, int max_new,
                int eos_id, int pad_id, void* stream);
/* tail of a decode step, one workgroup per row (csrc/select.hip): token selection — greedy, or temperature / top-k / top-p
 * sampling ([HF] generation/logits_process.py warpers + multinomial; serve/cli.py:122-132, serve/chat.py:141-151) — EOS /
 * pad / keyword-stop bookkeeping (mm_utils.py:128-151), embedding of the selected token (fp32 row x, RMSNorm partials ssq,
 * first GEMV operand xg = bf16(x * xg_w)) and the row's step / position advance (bit 0 / bit 1 of `advance`).  Every
 * per-row parameter lives in the row's record of `rows` ([nrows][vck_row_state_stride()] ints, csrc/kernels.h
 * RowStateField); row r writes its id to out_ids[rows[r][RS_OUT_OFF] + step]. */
void vck_select_embed(const float* logits, int ldl, int* rows, int* next_tok, int* out_ids, const uint16_t* embed, float* x,
                      float* ssq, const float* xg_w, uint16_t* xg, int D, int npart, int V, int nrows, int advance,
                      void* stream);
int vck_row_state_stride(void);
/* Prompt-lookup speculation, one workgroup per sequence (csrc/select.hip; records as above, sequence b = rows[b]).
 * vck_spec_draft: the corpus of a sequence is its lookup ids (lookup [B][lookup_stride], lookup_len [B]; NULL: none) | a separator
 * no window may touch | its prompt ids (prompt [B][prompt_stride], prompt_len [B] of them or, NULL, all; placeholders and all) | the
 * ids generated so far.  For ng = max_ngram .. 1
 * (an ng longer than prompt + generated is not tried) the last ng ids are sought at every earlier start; the latest match of the
 * first ng with a match decides; the ids behind it are the drafts — at most min(k, Q - 1, slots left - 1), cut at the corpus end and
 * at the first id outside [0, V).  tok [B * Q] = last emitted id, drafts, pad; nq [B] = 1 + drafts, 0 for an inactive, finished or
 * full row (whose token rows are pad).
 * vck_spec_accept: logits [B * Q, ldl]; a_j = argmax of row j (ties to the lower id); the leading drafts tok[j] == a_(j-1) are
 * accepted and a_0 .. a_n go one by one through the bookkeeping vck_select_embed applies to its token (EOS, stop sequences, the
 * row's last slot: a finishing token cuts the rest); words 2 / 3 of the record advance by the number emitted; next_tok[b] = the last
 * emitted id; counters [B][4] += {1, emitted, nq - 1, emitted - 1} (NULL: none).  lp_tok != NULL: the emitted rows' entries of
 * scratch_lp / scratch_ids ([B * Q, scratch_k], a vck_topk_logprob over the rows) go to the slabs at the ids' slots: lp_tok = entry 0,
 * lp_top / lp_ids = the first lp_k entries. */
void vck_spec_draft(const int* rows, const int* out_ids, const int* lookup, const int* lookup_len, int lookup_stride, const int* prompt,
                    const int* prompt_len, int prompt_stride, int* tok, int* nq, int B, int Q, int k, int max_ngram, int V, void* stream);
void vck_spec_accept(const float* logits, int ldl, int V, int* rows, int* next_tok, int* out_ids, const int* tok, const int* nq, int B,
                     int Q, int* counters, const float* scratch_lp, const int* scratch_ids, int scratch_k, float* lp_tok, float* lp_top,
                     int* lp_ids, int lp_k, void* stream);
/* vck_spec_accept with the rows' selections given: sel [B * Q] != NULL replaces the argmax (a_j = sel[b * Q + j]: what vck_spec_select
 * chose under sampling or on processed rows); scratch_chosen [B * Q] != NULL is the log-prob lp_tok takes for a_j (a vck_topk_logprob
 * with chosen = sel) instead of entry 0 of the scratch row.  Both NULL: vck_spec_accept. */
void vck_spec_accept_sel(const float* logits, int ldl, int V, int* rows, int* next_tok, int* out_ids, const int* tok, const int* nq, int B,
                         int Q, int* counters, const float* scratch_lp, const int* scratch_ids, int scratch_k, float* lp_tok, float* lp_top,
                         int* lp_ids, int lp_k, const int* sel, const float* scratch_chosen, void* stream);
/* the selections of a verify step: sel[b * Q + j] (j < nq[b]; other entries are not written) = what vck_select_embed would select from
 * logits row b * Q + j under record b with word 2 of the record (the step, the sampler's key) raised by j — greedy argmax or
 * temperature / top-k / top-p / Gumbel-max; no bookkeeping, the records are only read.  One workgroup per row, the rows side by side.
 * lds_floats: -1 = the scaled row is staged in LDS when the device allows, 0 = never (every pass re-reads global memory). */
void vck_spec_select(const float* logits, int ldl, int V, const int* rows, const int* nq, int* sel, int B, int Q, int lds_floats,
                     void* stream);
/* test hook of the sampler's warpers: keep[r * V + i] (int32 0 / 1) = whether the sampled selection of logits row r under record r can
 * draw token i — the set left by temperature -> top-k -> top-p -> min-p -> typical -> epsilon -> eta (record words 9 .. 11 and
 * 114 .. 117: 1 / temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff as float bits, zero = off for the last
 * four), computed by the threshold code vck_select_embed / vck_spec_select run.  Words 0 (active) and 8 (sample) are not looked at.
 * One workgroup per row; lds_floats as vck_spec_select takes it. */
void vck_warp_support(const float* logits, int ldl, int V, const int* rows, int nrows, int* keep, int lds_floats, void* stream);
/* test hook of the sampler: u[i] = the uniform in (0,1) the Gumbel-max draw derives from 32-bit hash h[i] (strictly
 * inside the interval for EVERY h, so the Gumbel term -log(-log(u)) written to gumbel[i] is finite) */
void vck_uniform_probe(const uint32_t* h, float* u, float* gumbel, int n, void* stream);
/* scoring: logprob[r] = logits[r, target[r]] - logsumexp(logits[r, 0:V]) over `rows` fp32 rows of stride ldl floats (ldl >= V; V and
 * the row starts need no alignment; columns V..ldl are never read).  -inf entries are legal while one entry of the row is finite; a
 * -inf target gives -inf.  target[r] in [0, V). */
void vck_token_logprob(const float* logits, int ldl, const int* target, float* logprob, int rows, int V, void* stream);
/* log-prob of a chosen token and the K most likely tokens of every row (generate(logprobs), score(top_logprobs)); rows as above.
 *   chosen_lp[r]    = logits[r, chosen[r]] - logsumexp(logits[r, 0:V]); a -inf logit gives -inf, chosen[r] < 0 gives 0.0
 *                     (chosen == NULL: every row 0.0; chosen_lp == NULL: not written)
 *   top_ids[r, 0:K], top_lp[r, 0:K]: the K largest logits of the row ordered by (value descending, id ascending) — ties break as
 *                     the greedy argmax breaks them — each as logit - logsumexp; when fewer than K entries are finite the
 *                     remaining slots hold id -1 and -inf.  K in 0 .. VC_MAX_TOP_LOGPROBS (K = 0: top_lp / top_ids untouched;
 *                     outside the range nothing is launched).
 * The log-prob of an id is the same expression wherever it appears: chosen_lp[r] is bit-equal to the top_lp entry of chosen[r].
 * The selection is exact (bisection over the order-preserving integer image of the values; -0.0 ties with +0.0).  lds_floats: LDS
 * floats the row may be staged in — < 0: what the device allows, 0 (or < V): every pass re-reads the row from global memory;
 * both paths give the same bits. */
#define VC_MAX_TOP_LOGPROBS 32
void vck_topk_logprob(const float* logits, int ldl, const int* chosen, float* chosen_lp, float* top_lp, int32_t* top_ids, int rows,
                      int V, int K, int lds_floats, void* stream);
/* One beam-search step of B sequences of n beams (rows b * n .. b * n + n - 1, R = B * n <= 16) behind a vck_topk_logprob with
 * K = 2 n into cand_lp / cand_id [R, 2 n]: candidate score = lp + beam_score[row] (one fp32 add), the 2 n best per sequence by
 * (score descending, then row, then id ascending; id -1 entries are no candidates), then HF's BeamSearchScorer.process (4.31): an id of
 * the EOS set at rank < n adds a hypothesis (score = sum / hyp_den[step]; at most n kept, the worst leaves), at rank >= n it is
 * skipped, anything else fills the next of the n beam slots; is_done with done_den[step] in the early_stopping mode.  Layouts:
 *   rows   [R][vck_row_state_stride()] RowState records: word 2 (step) is read, words 2 / 3 advance by advance & 1 / advance & 2
 *   seq    [B][4]: done, hypotheses held, float bits of the worst score (1e9 at the start), the step that set done
 *   hyp    [B][n][4]: float bits of score and of sum_logprobs, step, source row — back-pointers into
 *   tok_tab / parent_tab [max_new][R] (row `step` is written: the token and the source row of every row)
 *   params [12]: number of EOS ids (<= 8), pad id, early_stopping (0 false, 1 true, 2 "never"), max_new, 8 EOS ids
 *   flags  [2]: every sequence done (written each step); set when fewer than n beam slots could be filled (the host raises)
 * A done sequence emits pad with score 0, keeps its parents as the identity and ignores its candidates. */
void vck_beam_step(const float* cand_lp, const int* cand_id, float* beam_score, int* rows, int* next_tok, int* perm, int* tok_tab,
                   int* parent_tab, int* seq, int* hyp, const float* hyp_den, const float* done_den, const int* params, int* flags,
                   int B, int n, int advance, void* stream);
/* The beam loop's cache permutation: K and V of one layer, [R][H][cap_positions][pos_bytes] each; row r <- old row perm[r] for the
 * positions [start[r], rows[r] word 3 (position)) only, staged through tmp ([2][R][H][span_positions * pos_bytes] bytes; a longer
 * tail is cut at span_positions).  perm, start and the records are read on the device.  pos_bytes a multiple of 16. */
void vck_kv_permute_tail(void* kcache, void* vcache, void* tmp, const int* perm, const int* start, const int* rows, int R, int H,
                         int cap_positions, int pos_bytes, int span_positions, void* stream);
/* logits processors in front of the selection (generate(repetition_penalty=, no_repeat_ngram_size=, bad_words_ids=, min_new_tokens=)):
 * out[r, 0:V] = logits[r, 0:V] with the processors of row r applied; the raw rows are only read, columns V..ldo of `out` are not
 * written, the rows need no alignment (16-byte accesses where source and destination allow them).  One workgroup per row; the
 * parameters are the RowState record of the row (rows [nrows][128] int32, vck_row_state_stride()):
 *   [0] active (0: the row is skipped)   [2] step: ids generated so far   [4] max_new (the step is clamped to it)
 *   [5] EOS id (< 0: none)               [14] offset of the row's generated ids in out_ids
 *   [15] repetition penalty, float bits (> 0; 1.0 or 0 bits: off)        [96] no-repeat n-gram size (0: off)
 *   [97] min_new_tokens: while step < it, [5] and the ids of [102..] get -inf
 *   [98] / [99] offset and count of the row's prompt ids in prompt_ids   [100] how many sequences of bad_words apply to the row
 *   [101] count of further EOS ids (<= 8) in [102 .. 109]
 * The history of a row is its prompt ids followed by out_ids[off .. off + step).  In HF's order: the repetition penalty
 * (raw < 0 ? raw * p : raw / p, IEEE fp32, read from the raw row) over every history id, then -inf for every token that would
 * repeat an n-gram of the history, that completes a bad word (bad_words [32][9]: length 1 .. 8, ids; a one-id word always), and for
 * the EOS ids before min_new_tokens.  History and banned ids outside [0, V) are skipped (image placeholders). */
void vck_logits_process(const float* logits, int ldl, float* out, int ldo, const int* rows, const int* prompt_ids,
                        const int* out_ids, const int* bad_words, int nrows, int V, void* stream);
/* vck_logits_process with a token automaton behind the processors (constrained decoding; vcoder_amd/constraints.py): CSR tables —
 * state s owns the edges state_off[s] .. state_off[s + 1], edge_tok ascending and unique within a state, edge_next / default_next in
 * [-1, n_states).  Further record slots: [110] != 0: the automaton applies to the row; [111] / [112] the state behind the first
 * [112] ids of the row's out_ids (zeroes: the start state; -1: dead) — a cache the kernel advances to `step` and WRITES BACK, so
 * `rows` is not const here.  Unfinished rows only: every id without an edge in the row's state becomes -inf; a state whose
 * default_next >= 0 masks nothing; the dead state masks [0, V).  Edge ids outside [0, V) are ignored.  Null tables: exactly
 * vck_logits_process. */
void vck_logits_process_constrained(const float* logits, int ldl, float* out, int ldo, int* rows, const int* prompt_ids,
                                    const int* out_ids, const int* bad_words, const int* state_off, const int* edge_tok,
                                    const int* edge_next, const int* default_next, int n_states, int nrows, int V, void* stream);
/* the verify form (prompt-lookup speculation): logits / out hold B * Q rows; row b * Q + j (j < nq[b]; the others are not written) is
 * processed under record b with the drafts tok[b * Q + 1 .. b * Q + j] behind the record's history and step + j in place of its step
 * (min_new_tokens) — what vck_logits_process would write j steps later, had the drafts been emitted. */
void vck_logits_process_verify(const float* logits, int ldl, float* out, int ldo, const int* rows, const int* prompt_ids,
                               const int* out_ids, const int* bad_words, const int* tok, const int* nq, int B, int Q, int V, void* stream);
/* classifier-free guidance in front of the processors (generate(guidance_scale=, negative_prompt_ids=); HF's
 * UnbatchedClassifierFreeGuidanceLogitsProcessor): for every pair r of a raw conditional row c = cond[r] and a raw unconditional row
 * u = uncond[r] (fp32, stride ldl, finite)
 *   lc[t] = (c[t] - max c) - log(sum exp(c - max c)),   lu[t] likewise,   out[r, t] = g * (lc[t] - lu[t]) + lu[t]
 * in fp32 with the product and the sum rounded separately (no fused multiply-add); g = the float whose bits are word 113 of the
 * pair's RowState record (rows [nrows][vck_row_state_stride()]; word 0 == 0: the pair is skipped, nothing is written).
 * scalars[r] = {max c, log sum c, max u, log sum u}: `out` is an element-wise function of the two rows and these four values, which
 * numpy float32 reproduces bit for bit.  The raw rows are only read, nothing beyond column V - 1; columns V..ldo of `out` are not
 * written; the rows need no alignment (16-byte accesses where all three allow them).  One workgroup per pair. */
void vck_guidance_combine(const float* cond, const float* uncond, int ldl, float* out, int ldo, const int* rows, float* scalars,
                          int nrows, int V, void* stream);
/* the unconditional rows of a guided decode step follow their partners, behind vck_select_embed over rows 0 .. B - 1: row B + i takes
 * row i's next_tok, x row [D], ssq row [npart] and xg row [D]; word 1 of its record (finished) becomes row i's, and its OWN words
 * 2 / 3 (step / position) advance by advance & 1 / advance & 2.  A row B + i whose word 0 (active) is 0 and every row outside
 * [B, 2 B) are not touched.  D a multiple of 8 (else nothing is launched).  One workgroup per follower. */
void vck_guidance_follow(int* rows, int32_t* next_tok, float* x, float* ssq, uint16_t* xg, int B, int D, int npart, int advance,
                         void* stream);
void vck_embed_tokens_ssq(const int* tok, const uint16_t* embed, float* x, float* ssq, const float* xg_w, uint16_t* xg, int B,
                          int D, int npart, void* stream);
void vck_advance(int* step_dev, int* pos_dev, int* ctx_dev, void* stream);
/* strict (fp32-faithful) kernels behind vc_model_set_precision(m, 1): fp32 activations x bf16 weights on the exact
 * v_mfma_f32_16x16x4_f32, fp32 attention, fp32 head split + RoPE.  epi ids as vck_gemm (all outputs fp32). */
void vck_gemm_f32(const float* A, const uint16_t* W, const float* bias, float* out, int M, int N, int K, int lda, int ldw,
                  int ldo, int epi, void* stream);
void vck_attention_f32(const float* q, const float* k, const float* v, float* out, int B, int H, int Tq, int hd, int q_stride,
                       int kv_stride, int causal, int Tk, const int* pos0_dev, float scale, void* stream);
void vck_qkv_rope_f32(const float* qkv, float* q, float* k, float* v, int B, int T, int H, int hd, int q_stride, int kv_stride,
                      const int* pos0_dev, const float* rope_cos, const float* rope_sin, void* stream);
/* ---- precision mode "split" behind vc_model_set_precision(m, 2): the FAST kernels with every MFMA operand carried as two bf16
 * values, x = hi + lo (hi = bf16(x), lo = bf16(x - hi): ~16 mantissa bits; weights are exactly bf16), fp32 everywhere between
 * two MFMAs.  Meets the "logits within 1e-3, greedy ids bit-exact" bar of BASELINE.json at ~half the fast path's MFMA rate.
 * vck_gemm_split: A is [M, lda] with columns [0, Kw) = hi and [Kw, 2 Kw) = lo of the activation row; W [N, Kw] is contracted
 *   against both halves (its k index wraps); epi as vck_gemm; split_out > 0: bf16-valued epilogues write [hi | lo] again, the lo
 *   plane split_out columns to the right of the hi value.
 * vck_gemv_split: X is [G + M, K] — rows [0, M) hi, rows [G, G + M) lo (G = 8 for M <= 8, 16 for M <= 16); bf16-valued outputs
 *   (epi 0 / 3, xg_out) come back as hi row m + lo row G + m.
 * vck_*norm_split: normalised row r -> hi at y + r * ldy, lo at y + r * ldy + lo_off.
 * vck_qkv_split32: fp32 fused-QKV rows -> RoPE in fp32 -> fp32 K / V cache rows (k32 / v32, may be NULL) + bf16 hi / lo planes
 *   of Q [B,H,q_stride,hd], K [B,H,ks_stride,hd] and V^T [B,H,hd,vt_stride] (key order of vck_qkv_split's V^T).
 * vck_attention_split: flash attention over those planes (3 MFMAs per product), output rows [hi | lo]: stride ldo, lo at lo_off.
 * vck_attention_decode_kv32: the fused decode attention over fp32 qkv / fp32 K, V caches; output as stacked groups of G hi rows
 *   + G lo rows (row b -> hi at row (b / G) * 2G + b % G). */
void vck_gemm_split(const uint16_t* A, const uint16_t* W, const float* bias, void* out, int M, int N, int Kw, int lda, int ldo,
                    int epi, int split_out, float* ws, size_t ws_bytes, void* stream);
void vck_gemv_split(const uint16_t* X, const void* Wp, const float* wscale, void* out, const float* ssq_in, float* ssq_out,
                    const float* xg_w, uint16_t* xg_out, int npart, float eps, int M, int N, int K, int ldo, int epi, int G,
                    void* stream);
/* the decode GEMV with every argument: G = split rows (0: bf16 step; 8 / 16 / 32: X holds hi rows [0, M) and lo rows [G, G + M)),
 * the split-K buffers and their capacity (floats / counters; 0 = the historical [4][512][2][256] / [512][2]) */
void vck_gemv_full(const uint16_t* X, const void* Wp, const float* wscale, void* out, const float* ssq_in, float* ssq_out,
                   const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch, unsigned long long sk_scratch_floats,
                   unsigned* sk_counters, int sk_counters_n, int ksplit, int M, int N, int K, int ldo, int epi, int G, void* stream);
/* Inexact checkpoints (fp16 / fp32 values bf16 cannot hold; vc_model_inexact_tensors): w = bf16 hi + bf16 lo.
 *  vck_f32_to_bf16_planes: hi = bf16(in), lo = bf16(in - hi) (lo may be NULL), *inexact = 1 if any in != hi
 *  vck_gemm_f32_wlo:   the strict GEMM over W + W_lo
 *  vck_gemm_split_wlo: the split prefill GEMM with a third K segment a_hi . w_lo (W_lo [N, Kw] like W; NULL = vck_gemm_split)
 *  vck_gemv_split_wlo: the split decode GEMV (G > 0, workgroup-shared form) with the packed lo plane */
void vck_f32_to_bf16_planes(const float* in, uint16_t* hi, uint16_t* lo, uint64_t n, unsigned* inexact, void* stream);
void vck_gemm_f32_wlo(const float* A, const uint16_t* W, const uint16_t* W_lo, const float* bias, float* out, int M, int N, int K,
                      int lda, int ldw, int ldo, int epi, void* stream);
void vck_gemm_split_wlo(const uint16_t* A, const uint16_t* W, const uint16_t* W_lo, const float* bias, void* out, int M, int N, int Kw,
                        int lda, int ldo, int epi, int split_out, float* ws, size_t ws_bytes, void* stream);
void vck_gemv_split_wlo(const uint16_t* X, const void* Wp, const void* Wp_lo, void* out, const float* ssq_in, float* ssq_out,
                        const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch, unsigned long long sk_scratch_floats,
                        unsigned* sk_counters, int sk_counters_n, int ksplit, int M, int N, int K, int ldo, int epi, int G, void* stream);
/* which kernel serves the decode GEMV of precision mode "split": 0 = per-wave rings (gemv_dma_kernel; two weight passes of 16
 * rows per 32-row step), 1 / -1 (default) = workgroup-shared activation chunks (gemv_wg_kernel; hi + lo planes in one pass) with
 * four or six tiles per workgroup as the launcher chooses per matrix; 2 = four everywhere (A/B), 3 = six everywhere (tests) */
void vck_set_gemv_variant(int v);
/* K12 + K13 + K14 in one launch (round 6): the fused-QKV projection of a prefill layer whose epilogue applies RoPE, splits the heads
 * and writes Q [B,H,q_stride,128], roped K rows and V rows [B,H,kv_stride,128] (and / or their e4m3 cache rows k8 / v8
 * [B,H,kv8_stride,128]) and the V^T scratch [B,H,128,vt_stride] in the flash kernel's key order — bit for bit what vck_gemm
 * (EPI_BF16) + vck_qkv_split_kv / _kv8 produce.  A [B * T, lda] bf16, W [3 * H * 128, K] bf16 (HF q / k / v rows stacked); f8 != 0:
 * A and W are e4m3 bytes with a_scale [B * T] / w_scale [3 * H * 128].  (H * 128) % 256 == 0.  ws: optional split-K workspace. */
void vck_gemm_qkv(const void* A, const float* a_scale, const void* W, const float* w_scale, const float* bias, int B, int T, int H, int K,
                  int lda, uint16_t* q, uint16_t* k, uint16_t* v, uint16_t* vt, uint8_t* k8, uint8_t* v8, int q_stride, int kv_stride,
                  int vt_stride, int kv8_stride, const float* rope_cos, const float* rope_sin, int f8, float* ws, size_t ws_bytes,
                  void* stream);
/* test hook, inside one process: on != 0 sends the bf16 GEMMs of every size to the 8-phase 256 x 256 kernel (default 0: only
 * M >= 1024 and N >= 512; the e4m3 and fused-QKV GEMMs always take it) */
void vck_set_gemm_force_8phase(int on);
/* launches the GEMM launcher has sent to the 128 x 128 LDS-DMA kernel / to the 8-phase 256 x 256 kernel (the e4m3 and fused-QKV
 * forms included; a split-K fix-up launch is not counted) since the library was loaded (tests) */
unsigned long long vck_gemm_dma_launches(void);
unsigned long long vck_gemm_8phase_launches(void);
/* NT = ceil(tiles / 256) tiles per workgroup for bf16 matrices of more than 512 tiles, one deep-ringed workgroup per CU (NT in
 * 3, 4, 6, 7): -1 / 1 = the classes that measured faster (default), 0 = off, 2 = every class.  Results are bit-identical
 * whichever is set. */
void vck_set_gemv_wide(int v);
unsigned long long vck_gemv_wide_launches(void);
unsigned long long vck_gemv_wg_launches(void);   /* launches the workgroup-shared form has served (tests) */
/* the geometry the decode GEMV launcher chooses for a call (vck_gemv_full's arguments; of the optional buffers only their presence:
 * fp8 = W8A16 weights, has_sk = the split-K buffers with the given capacities, has_wlo = a weight lo plane) under the current
 * vck_set_gemv_variant / vck_set_gemv_wide values, without launching.  Returns 0 and out = {form (0 ring, 1 wide, 2 workgroup-shared),
 * waves, tiles per workgroup (per wave in form 2), ring slots, 8-row activation pieces, chunk lines (form 2), fp8, wlo, K-slices,
 * workgroups}, or -1 where the launcher refuses the call (tests: tests/golden/gemv_plan.npz pins the table) */
int vck_gemv_plan(int M, int N, int K, int epi, int fp8, int split_rows, int ksplit, int has_sk, unsigned long long sk_scratch_floats,
                  int sk_counters_n, int has_wlo, int out[10]);
/* W4A16 decode weights: MXFP4.  Per output row and per block of 32 consecutive k: e = the smallest integer with max|block| <= 6 * 2^e
 * (>= -13; 0 for an all-zero block), stored as the E8M0 byte e + 127 in scale [N/16][K/128][64 lanes]; elements q = e2m1(W / 2^e)
 * (nearest, ties to the even code) as nibbles in Wq [N/16][K/128][64 lanes][16 B], lane = n%16 + 16*((k%128)/32), k even in the low
 * nibble of a byte; W [N,K] is overwritten with the effective weights q * 2^e (exact in bf16 and in fp16).  K % 128 == 0, N % 16 == 0.
 * vcoder_amd/quant.py (quantize_blocks_mxfp4, pack_w4) states the same on the host. */
void vck_quantize_mxfp4(uint16_t* W, uint8_t* Wq, uint8_t* scale, int N, int K, void* stream);
/* vck_gemv_ex over those nibbles and scale bytes (a kernel of its own: four waves split K in 128-wide super-tiles); ksplit > 1 needs
 * the hand-off buffers.  vck_gemv_w4_split: precision mode "split", X = [G + M, K] hi rows then lo rows (G = 8: M <= 8, 16: M <= 16). */
void vck_gemv_w4(const uint16_t* X, const void* Wq, const uint8_t* w4scale, void* out, const float* ssq_in, float* ssq_out,
                 const float* xg_w, uint16_t* xg_out, int npart, float eps, float* sk_scratch, unsigned* sk_counters, int ksplit, int M,
                 int N, int K, int ldo, int epi, void* stream);
void vck_gemv_w4_split(const uint16_t* X, const void* Wq, const uint8_t* w4scale, void* out, const float* ssq_in, float* ssq_out,
                       const float* xg_w, uint16_t* xg_out, int npart, float eps, int M, int N, int K, int ldo, int epi, int G, void* stream);
/* what those would launch: 0 and out = {form (3), waves, tiles per workgroup, ring slots, 8-row activation pieces, K-slices,
 * workgroups}, or -1 where the launcher refuses the call.  vck_set_gemv_w4_nt: 0 = tiles per workgroup by the tile count (default),
 * 1 / 2 / 4 = for every matrix (tests, A/B; the bits do not depend on it). */
int vck_gemv_w4_plan(int M, int N, int K, int epi, int split_rows, int ksplit, int has_sk, int out[7]);
void vck_set_gemv_w4_nt(int nt);
void vck_rmsnorm_split(const float* x, const int* row_idx, const float* w, uint16_t* y, int rows, int D, float eps, int ldy,
                       uint64_t lo_off, void* stream);
void vck_layernorm_split(const float* x, const float* w, const float* b, uint16_t* y, int rows, int D, float eps, int ldy,
                         uint64_t lo_off, void* stream);
void vck_qkv_split32(const float* qkv, uint16_t* q_hi, uint16_t* q_lo, uint16_t* k_hi, uint16_t* k_lo, uint16_t* vt_hi,
                     uint16_t* vt_lo, float* k32, float* v32, int B, int T, int H, int hd, int q_stride, int ks_stride, int vt_stride,
                     int kv_stride, const float* rope_cos, const float* rope_sin, void* stream);
void vck_attention_split(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                         const uint16_t* vt_hi, const uint16_t* vt_lo, uint16_t* out, int B, int H, int T, int hd, int q_stride,
                         int kv_stride, int causal, float scale, int ldo, int lo_off, void* stream);
void vck_attention_decode_kv32(const float* qkv, float* k, float* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                               const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                               const float* rope_sin, float scale, int G, void* stream);
/* fp24 KV caches of precision mode "split" (rows of hd x u16 | hd x u8: the top 24 bits of the fp32 values, RNE — 0.75 of the fp32
 * bytes at 2^-17 relative precision): the writer of a prefill and the fused decode attention over them */
void vck_qkv_split24(const float* qkv, uint16_t* q_hi, uint16_t* q_lo, uint16_t* k_hi, uint16_t* k_lo, uint16_t* vt_hi,
                     uint16_t* vt_lo, void* k24, void* v24, int B, int T, int H, int hd, int q_stride, int ks_stride, int vt_stride,
                     int kv_stride, const float* rope_cos, const float* rope_sin, void* stream);
void vck_attention_decode_kv24(const float* qkv, void* k, void* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                               const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                               const float* rope_sin, float scale, int G, void* stream);
/* e4m3 KV caches of the fp8 weight format (rows of hd bytes, no scale, saturating at 448): the prefill's writer (the bf16 K rows go to
 * a per-call scratch for the flash kernel) and the bf16 decode step's fused attention over them */
void vck_qkv_split_kv8(const uint16_t* qkv, uint16_t* q, uint16_t* k, uint8_t* k8, uint8_t* v8, uint16_t* vt, int B, int T, int H, int hd,
                       int q_stride, int kv_stride, int vt_stride, int kv8_stride, const float* rope_cos, const float* rope_sin,
                       void* stream);
void vck_attention_decode_kv8(const uint16_t* qkv, uint8_t* k, uint8_t* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                              const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                              const float* rope_sin, float scale, void* stream);
/* ---- the attention kernels with the arguments the engine sets for padded batches and for a prefill into a cache (tests).
 * key_mask [B][mask_stride] bytes: key_mask[b * mask_stride + key] == 0 hides that key from every query of sequence b (NULL = no
 * mask; key 0 must be visible, and for the decode step the row's own position).  Bytes at keys the launch does not reach are
 * never read.
 * vck_attention_ex: vck_attention with V^T rows of their own stride (vt_stride columns, a multiple of 64; 0 = kv_stride) — the LLM
 *   prefill's form: q_stride = S, kv_stride = the cache capacity, vt_stride = S rounded up to 64 — and a key mask.
 * vck_attention_split_ex: vck_attention_split likewise.
 * vck_attention_decode_masked: the per-row fused decode attention (vck_attention_decode_rows / _kv32 / _kv24 / _kv8) over the cache
 *   format kv_format — 0 bf16, 1 fp32, 2 fp24, 3 e4m3; qkv is fp32 and G the output row group for 1 and 2 — with a mask per row.
 * vck_attention_f32_masked: vck_attention_f32 with a key mask.
 * vck_attn_probs: output_attentions — probabilities out [B,H,T,Tk'] fp32 (Tk' = Tk, or T when Tk == 0) of T queries at positions
 *   q_pos0 + t over keys 0 .. q_pos0 + t ([HF] llama eager_attention_forward :191-214 attn_weights); hidden and future keys get 0.
 *   q: q32 [B,H,q_stride,hd] fp32, or bf16 q_hi (+ q_lo: hi + lo planes); k rows [B,H,kv_stride,hd]: k32 fp32, or bf16 k_hi (+ k_lo),
 *   or e4m3 bytes k8, or fp24 rows k24 (the first non-NULL of k32, k8, k_hi, k24 is used).  keys <= 4096. */
void vck_attention_ex(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* out, int B, int H, int T, int hd,
                      int q_stride, int kv_stride, int vt_stride, int causal, float scale, const uint8_t* key_mask, int mask_stride,
                      void* stream);
void vck_attention_split_ex(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* k_hi, const uint16_t* k_lo,
                            const uint16_t* vt_hi, const uint16_t* vt_lo, uint16_t* out, int B, int H, int T, int hd, int q_stride,
                            int kv_stride, int vt_stride, int causal, float scale, int ldo, int lo_off, const uint8_t* key_mask,
                            int mask_stride, void* stream);
void vck_attention_decode_masked(const void* qkv, void* k, void* v, uint16_t* out, int B, int H, int hd, int kv_stride,
                                 const int* pos_rows, int pos_stride, const int* active_rows, const float* rope_cos,
                                 const float* rope_sin, float scale, int kv_format, int G, const uint8_t* key_mask, int mask_stride,
                                 void* stream);
void vck_attention_f32_masked(const float* q, const float* k, const float* v, float* out, int B, int H, int Tq, int hd, int q_stride,
                              int kv_stride, int causal, int Tk, const int* pos0_dev, float scale, const uint8_t* key_mask,
                              int mask_stride, void* stream);
void vck_attn_probs(const float* q32, const uint16_t* q_hi, const uint16_t* q_lo, const float* k32, const uint16_t* k_hi,
                    const uint16_t* k_lo, const void* k24, const uint8_t* k8, float* out, int B, int H, int T, int hd, int q_stride,
                    int kv_stride, float scale, int Tk, int q_pos0, const uint8_t* key_mask, int mask_stride, void* stream);
/* deterministic synthetic tensors (vcoder_amd/synth.py) and dtype converts */
void vck_synth_bf16(uint16_t* out, uint64_t n, uint32_t tseed, float offset, float halfwidth, void* stream);
void vck_synth_f32(float* out, uint64_t n, uint32_t tseed, float offset, float halfwidth, void* stream);
/* the generator's value before the bf16 rounding, as an fp16 checkpoint holds it (rounding 1) or unrounded fp32 (2):
 * vcoder_amd/synth.py synth_tensor(rounding="fp16" | "fp32") */
void vck_synth_f32_rounded(float* out, uint64_t n, uint32_t tseed, float offset, float halfwidth, int rounding, void* stream);
void vck_f32_to_bf16(const float* in, uint16_t* out, uint64_t n, void* stream);
void vck_bf16_to_f32(const uint16_t* in, float* out, uint64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
