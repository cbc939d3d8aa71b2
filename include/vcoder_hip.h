/* vcoder_hip.h — C ABI of libvcoder_hip.so: the MI355X-native VCoder inference hot path.
 *
 * The reference (SHI-Labs/VCoder) has no FFI: its boundary is the Python model API
 *   load_pretrained_model()                     vcoder_llava/model/builder.py:25-154
 *   VCoder[DS]LlavaLlamaForCausalLM.forward()   vcoder_llava/model/language_model/vcoder_ds_llava_llama.py:57-118
 *   .generate() (HF GenerationMixin)            called at vcoder_llava/serve/cli.py:122-132
 * This library owns all device work behind that API; vcoder_amd/ (Python, ctypes) re-creates the
 * reference's import surface on top of it.  Plain C: opaque handles, pointers and sizes,
 * no C++ types, no exceptions across the boundary.
 *
 * Ownership: the caller owns every input/output buffer; the library owns weights, KV cache, workspaces,
 * streams and hipGraph objects.  `vc_model_load_tensor` copies (the caller may free immediately).
 * Threading: one vc_model = one device + one stream; not thread-safe (matches the reference's callers).
 * Errors: every call returns VC_OK (0) or a negative vc_status; vc_last_error() gives the message.
 */
#ifndef VCODER_HIP_H
#define VCODER_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vc_ctx vc_ctx;
typedef struct vc_model vc_model;

typedef enum {
    VC_OK = 0,
    VC_IGNORED = 1,          /* load_tensor: key accepted but dead at inference */
    VC_ERR_INVALID = -1,     /* bad argument / shape / unknown key            -> ValueError   */
    VC_ERR_HIP = -2,         /* HIP runtime failure                           -> RuntimeError */
    VC_ERR_STATE = -3,       /* call order violation (e.g. decode before prefill) -> RuntimeError */
    VC_ERR_INDEX = -4,       /* a placeholder id reached the embedding lookup -> IndexError (vcoder_llava_arch.py:187 quirk) */
    VC_ERR_UNEQUAL = -5      /* unequal spliced lengths with attention_mask   -> UnboundLocalError (vcoder_ds_llava_arch.py:295-297) */
} vc_status;

/* which reference class: llava_arch.py / vcoder_llava_arch.py / vcoder_ds_llava_arch.py */
typedef enum { VC_VARIANT_LLAVA = 0, VC_VARIANT_VCODER = 1, VC_VARIANT_VCODER_DS = 2 } vc_variant;
typedef enum { VC_F32 = 0, VC_BF16 = 1 } vc_dtype;
typedef enum { VC_MOD_IMAGE = 0, VC_MOD_SEG = 1, VC_MOD_DEPTH = 2 } vc_modality;

/* Mirrors the config keys the reference constructors read. */
typedef struct vc_model_cfg {
    int32_t variant;            /* vc_variant */
    /* CLIP ViT (multimodal_encoder/clip_encoder.py) */
    int32_t vit_hidden, vit_heads, vit_ffn, vit_layers, vit_layers_used, vit_image, vit_patch;
    int32_t vit_keep_cls;       /* mm_vision_select_feature == 'cls_patch' */
    float vit_ln_eps;
    /* Llama decoder */
    int32_t hidden, heads, ffn, layers, vocab, max_positions;
    float rms_eps, rope_theta;
    /* adapters: 0 = identity, 1 = linear, N = mlpNx_gelu  (multimodal_projector/builder.py:33-51) */
    int32_t mm_proj_depth, seg_proj_depth;
    int32_t pad_token_id;
} vc_model_cfg;

/* ---- lifetime ------------------------------------------------------------------------------ */
int vc_init(int device_id, vc_ctx** out);
void vc_shutdown(vc_ctx* ctx);
const char* vc_last_error(vc_ctx* ctx);
int vc_synchronize(vc_ctx* ctx);
void* vc_stream(vc_ctx* ctx);                 /* the hipStream_t all work of this context is enqueued on */

int vc_model_create(vc_ctx* ctx, const vc_model_cfg* cfg, vc_model** out);
void vc_model_destroy(vc_model* m);
/* another session (own stream = `ctx`, own KV cache / workspaces / graph) on the finalized weights of `parent`,
 * shared read-only; `parent` must outlive it.  Sessions on different contexts may run concurrently. */
int vc_model_create_shared(vc_ctx* ctx, vc_model* parent, vc_model** out);

/* ---- weights: replaces HF from_pretrained() of builder.py:93-108 + CLIPVisionTower.load_model() ---- */
/* hf_key = state-dict key of the reference checkpoint; host_ptr = row-major tensor of `dtype`; the full shape is checked
 * (a transposed matrix is an error, not a silent load). */
int vc_model_load_tensor(vc_model* m, const char* hf_key, const void* host_ptr, int dtype, const int64_t* shape,
                         int ndim);
/* device-side deterministic generator, bit-identical to vcoder_amd/synth.py:synth_tensor (benchmarks, tests) */
int vc_model_synth_tensor(vc_model* m, const char* hf_key, const int64_t* shape, int ndim, uint32_t tensor_seed,
                          float offset, float halfwidth);
/* after the last tensor: fuses QKV / interleaves gate-up / packs decode copies; fails listing a missing key */
/* on = 1: a sample's results do not depend on the batch (or the rank's shard) it runs in — the prefill GEMMs skip their split-K
 * remainder round, whose slicing follows the tile count; everything else already is batch-invariant.  The reference's rows are
 * independent of the batch size; with it the ids of N ranks x B equal those of one rank x N B bit for bit.
 * Costs a short last round of tiles per GEMM.  Default 0.  Applies to every session of the model. */
int vc_model_set_batch_invariant(vc_model* m, int on);
/* Round 6: the prefill's QKV GEMM applies RoPE, splits the heads and writes Q / the KV-cache rows / the V^T scratch in its epilogue
 * (replaces [HF] llama/modeling_llama.py:254-262 "q/k/v_proj -> view -> apply_rotary_pos_emb -> cache update" as ONE launch); default 1.
 * 0 = the separate GEMM + split launches of rounds 1-5 (regression / A-B); 1 = fused from 1024 token rows (where the 256 x 256 GEMM
 * kernel runs anyway); 2 = fused for every problem size.  Needs head_dim 128 and hidden_size % 256 == 0, else the separate launches. */
int vc_model_set_qkv_fused(vc_model* m, int on);
/* weight format 2 ("fp8"): KV cache of the decode steps in e4m3 (default 1) or bf16 (0).  Before vc_model_finalize. */
int vc_model_set_fp8_kv(vc_model* m, int on);
/* vc_model_synth_tensor with the value classes of the reference's checkpoints: rounding 0 bf16, 1 fp16-valued, 2 unrounded fp32
 * (vcoder_amd/synth.py synth_tensor(rounding=...)); 1 and 2 take the fp32 load path and keep weight lo planes */
int vc_model_synth_tensor_rounded(vc_model* m, const char* hf_key, const int64_t* shape, int ndim, uint32_t tensor_seed, float offset,
                                  float halfwidth, int rounding);
int vc_model_finalize(vc_model* m);
/* Number of loaded tensors whose fp32 source held values bf16 cannot represent — the reference's own checkpoints: an fp16 LLM
 * (model/builder.py:25-40, torch_dtype=float16) and an fp32 CLIP hub checkpoint (multimodal_encoder/clip_encoder.py:22-27).  Every
 * such matrix keeps a second bf16 plane lo = bf16(w - bf16(w)); precision modes "strict" and "split" contract against hi + lo (the
 * checkpoint's values to ~16 mantissa bits; exact for fp16 values), the bf16 fast path uses the bf16-rounded weights alone.
 * 0 for a bf16 checkpoint.  >= 0, or a negative vc_status. */
int vc_model_inexact_tensors(vc_model* m);
/* Round 6: which 16-bit format the MFMA operands / stored activations of THIS library have: 0 = bfloat16 (libvcoder_hip.so), 1 = IEEE
 * fp16 (libvcoder_hip_f16.so — same sources, same C ABI, built with -DVC_F16: fp16 operands on v_mfma_f32_16x16x32_f16 at the bf16
 * rate, conversions saturating at 65504; the operand precision of the reference's own GPU path, vcoder_llava/model/builder.py:39
 * torch_dtype=float16 and :142).  "bf16" in the names and comments of this header then reads "the library's operand format": an
 * fp16-valued checkpoint is held exactly (vc_model_inexact_tensors counts what fp16 cannot hold). */
int vc_operand_format(void);

/* arithmetic mode: 0 = bf16 MFMA operands, fp32 accumulate/residual/softmax (default; what bench.py measures);
 * 1 = strict: fp32 activations end to end on fp32 MFMA (slow) — within ~1e-5 of the reference's fp32 CPU path;
 * 2 = split: fp32 activations in HBM, every MFMA operand carried as two bf16 values (x = hi + lo, ~16 mantissa bits) on the
 *     FAST kernels — GEMMs contract the [hi | lo] rows against the (exactly bf16) weight twice, attention uses three MFMAs per
 *     product, fp24 KV cache (the top 24 bits of the fp32 values; VC_SPLIT_KV=32: fp32), one weight pass per 32-row pooled
 *     decode step; runs in sessions, the hipGraph loop and the decode pool at 0.60 of the bf16 path's rate.
 * 1 and 2 meet the "logits within 1e-3, greedy ids bit-exact" bar of BASELINE.json (2: 1.9e-4 at full 7b depth over 128
 * tokens, every greedy id equal to the fp32 reference's; the same at 13b, B = 16).  Takes effect at the next prefill. */
int vc_model_set_precision(vc_model* m, int mode);

/* parity diagnostic: prefills evaluate only the first n decoder layers (0 = all), final norm + lm_head applied to that
 * hidden state — error growth with depth is measured on one loaded model (tests/test_gpu_fulldepth.py) */
int vc_model_set_layer_limit(vc_model* m, int n_layers);

/* parity diagnostic (per-layer teacher forcing): decoder layers [l0, l1) of a prefill applied to a caller-supplied residual
 * stream x_in [B, S, hidden] (host fp32, positions 0..S-1) in the model's weight format / precision mode; x_out [B, S, hidden]
 * = the residual stream behind layer l1 - 1.  Every layer can be fed the oracle's own input, so that rounding / quantisation
 * noise of the layers in front of it does not compound (tests/test_gpu_e2e.py: fp8 formats per layer). */
int vc_debug_prefill_layers(vc_model* m, int l0, int l1, const float* x_in, int B, int S, float* x_out);
/* Test hook: captures of a decode step (hipGraph) the session's own loop has performed so far — vc_decode_step, vc_generate* on the
 * session, vc_generate_beam; the shared pool's are not counted.  A call that replays the step it finds adds 0. */
int vc_debug_step_captures(vc_model* m);

/* decoder weight storage: 0 = bf16 (default); 1 = W8A16 — the seven linears of every decoder layer are quantised at
 * vc_model_finalize to OCP fp8 e4m3 with one power-of-two scale per output row and streamed as bytes by the decode
 * GEMV (half the HBM traffic of the decode step); the prefill GEMMs read the same dequantised values in bf16, so both
 * phases compute with one set of effective weights.  2 = fp8, BASELINE.json configs[4] ("fp8 weights, CDNA4 fp8 MFMA"):
 * the weights and decode steps of 1, and the prefill's decoder linears quantise their activation rows to e4m3 (one
 * power-of-two scale per token row) and run e4m3 x e4m3 on v_mfma_scale_f32_16x16x128_f8f6f4 (W8A8, twice the bf16
 * MFMA rate), and the KV cache holds e4m3 rows (no scale, saturating; vc_model_set_fp8_kv(m, 0) before vc_model_finalize: bf16 rows) — half the bytes of the stream
 * that dominates the pooled 13b decode step.  The reference's counterpart is `load_8bit` (builder.py:31-33, bitsandbytes LLM.int8 — also 8-bit
 * weights x 8-bit activations).  3 = W4A16: the same seven linears as MXFP4 — OCP e2m1 elements with one power-of-two (E8M0) scale per
 * 32 consecutive k of a row — streamed as nibbles + scale bytes by the decode GEMV (0.53 bytes per weight) and widened exactly in
 * registers; as with 1, the row-major matrices are rewritten with the effective weights q * 2^e (exact in bf16 and in fp16), so every other
 * path computes with what decode sees.  Needs hidden_size and intermediate_size divisible by 128 (refused at vc_model_finalize otherwise).
 * This is not the reference's `load_4bit` (bitsandbytes NF4).  Call before vc_model_finalize. */
int vc_model_set_weight_format(vc_model* m, int fmt);

/* ---- hot path ------------------------------------------------------------------------------ */
/* encode_images / encode_seg_images / encode_depth_images (vcoder_ds_llava_arch.py:106-119):
 * pixels fp32 [B,3,S,S] (host, or device when pixels_on_device) -> projected features fp32 [B,P,hidden] on host. */
int vc_encode(vc_model* m, int modality, const float* pixels, int pixels_on_device, int B, float* out_feats_host);

/* CLIPVisionTower.forward + feature_select (vcoder_llava/model/multimodal_encoder/clip_encoder.py:29-51): the un-projected
 * tower output the reference's encode_* hand to the adapters — hidden_states[mm_vision_select_layer] of N images with the
 * CLS row dropped for 'patch'.  pixels fp32 [N,3,S,S] -> out fp32 [N, R, vit_hidden] on the host (R = patches, +1 for
 * 'cls_patch'). */
int vc_vision_tower_forward(vc_model* m, const float* pixels, int pixels_on_device, int N, float* out_host);

/* images per sample for the NEXT vc_prefill* / vc_generate* call (one-shot): the reference's list / 5-D image form
 * (vcoder_ds_llava_arch.py:135-169) — sample b owns counts[b] images of a modality, whose feature rows are spliced as ONE
 * block at its placeholder; the pixel pointer of that modality then holds sum(counts) images.  NULL = one per sample. */
int vc_set_image_counts(vc_model* m, const int32_t* img_counts, const int32_t* seg_counts, const int32_t* depth_counts, int B);

/* output_hidden_states for the NEXT vc_prefill (one-shot): out (host, cap_floats floats) receives [(layers + 1), B, S, hidden]
 * fp32 — inputs_embeds, the residual stream behind every decoder layer, the last entry after the final RMSNorm: the tuple
 * [HF] LlamaModel.forward returns as hidden_states (vcoder_ds_llava_llama.py:81-90,117).  out must stay valid until that
 * vc_prefill returns; NULL cancels.  Requested before a vc_decode_step instead, it is that cached step's tuple:
 * [(layers + 1), B, 1, hidden] (the step then runs eagerly, outside its hipGraph). */
int vc_request_hidden_states(vc_model* m, float* out, size_t cap_floats);

/* output_attentions for the NEXT vc_prefill (one-shot): out (host, cap_floats floats) receives [layers, B, heads, S, S] fp32 — the
 * attention probabilities HF's eager attention returns as `attentions` (vcoder_ds_llava_llama.py:81-90,118; [HF]
 * llama/modeling_llama.py eager_attention_forward): softmax(q k^T / sqrt(hd) + causal mask + padding mask), recomputed per layer
 * from that layer's q / k by a diagnostic kernel (the flash kernels never materialise them).  S <= 4096.  Requested before a
 * vc_decode_step: [layers, B, heads, 1, pos + 1] — the new token's query over every cached key and itself. */
int vc_request_attentions(vc_model* m, float* out, size_t cap_floats);

/* Padded batches: the caller's 2-D attention_mask [B, T] (bytes, 0 = hidden) for the NEXT vc_prefill* / vc_generate* call
 * (one-shot).  As in the reference, it is LEFT-extended with "visible" over the S - T rows the splice adds — by position
 * (vcoder_ds_llava_arch.py:305-311) — and a hidden position is hidden as a KEY from every query of its sequence during the
 * prefill ([HF] LlamaModel: causal mask + padding mask); position ids stay arange(S).  Spliced lengths must be equal (quirk 6)
 * and position 0 visible.  Cached steps: vc_generate* runs them under an all-ones mask, like the reference's multimodal decode
 * path (vcoder_ds_llava_arch.py:130-133 replaces the mask by ones: the padded positions' keys become visible); a vc_prefill +
 * vc_decode_step loop keeps the prefill's hidden keys hidden (a caller carrying its mask through the steps) until
 * vc_clear_attention_mask(). */
int vc_set_attention_mask(vc_model* m, const uint8_t* mask, int B, int T);
int vc_clear_attention_mask(vc_model* m);

/* KV-cache slots the next vc_prefill keeps free behind the prompt for vc_decode_step loops (default 64, clamped to
 * max_position_embeddings).  A loop that outruns the reserve still works: the cache grows (one copy of the live prefix). */
int vc_model_reserve_decode(vc_model* m, int max_new_tokens);

/* prepare_inputs_labels_for_multimodal + LlamaModel + lm_head (vcoder_ds_llava_llama.py:57-118), prefill.
 * ids [B,T] int64 host with -200/-300/-400 placeholders; seg/depth may be NULL.  has_attention_mask only
 * selects the reference's behaviour for unequal spliced lengths (error vs zero right-padding).
 * logits_last [B,V] and/or logits_all [B,S,V] (host fp32) may be NULL.  Leaves the KV cache at length S. */
int vc_prefill(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
               int pixels_on_device, int has_attention_mask, float* logits_last, float* logits_all, int* S_out);
/* encode + splice only: inputs_embeds [B,S,hidden] fp32 to host (what prepare_inputs_labels_for_multimodal returns) */
int vc_prefill_embeds_only(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                           const float* depth, int pixels_on_device, int has_attention_mask, float* out_host,
                           int* S_out);
/* the spliced length S the same arguments would give a vc_prefill / vc_generate call — the splice plan of
 * prepare_inputs_labels_for_multimodal (vcoder_ds_llava_arch.py:175-276) alone: no tower pass, no KV / mask state touched;
 * img / seg only say whether the modality is present, the depth pixels are read for is_depth_zero (:161).  Same plan errors
 * (VC_ERR_INDEX, VC_ERR_UNEQUAL) as the real call. */
int vc_plan_spliced_len(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                        int pixels_on_device, int has_attention_mask, int* S_out);

/* one cached decode step (input_ids.shape[1]==1 fast path, vcoder_ds_llava_arch.py:130-133).
 * tok [B] host (NULL: use the token the previous step selected on device); logits [B,V] host or NULL;
 * next_tok [B] host (greedy argmax, lowest index on ties) or NULL. */
int vc_decode_step(vc_model* m, const int32_t* tok, float* logits, int32_t* next_tok);

/* multi-token continuation of a cached sequence (HF LlamaModel over past_key_values with n > 1 new ids, no images): tok [B, n]
 * host, B = the batch of the last vc_prefill, at positions P .. P+n-1 (P = the loop's position), causal inside the chunk, every
 * cached key visible except those the prefill's attention_mask hides (while vc_decode_step would hide them).  logits_all
 * [B, n, V] host or NULL; logits_last [B, V] (row n-1 of each sequence) host or NULL.  Honours vc_request_hidden_states
 * ([(layers + 1), B, n, hidden]) and vc_request_attentions ([layers, B, heads, n, P+n]).  Afterwards the loop stands at P + n:
 * vc_decode_step continues there (tok = NULL: from the greedy choice of the last logits), vc_reorder_cache applies, a cache
 * that runs past its reserve grows.  Precision mode "bf16": the extend path (attention over the cache with n queries per
 * head, GEMV linears up to 128 rows, GEMMs above); "strict" / "split": n cached steps, bit-identical to n vc_decode_step
 * calls.  A refused call (bad ids, shape, state) changes nothing. */
int vc_extend(vc_model* m, const int32_t* tok, int B, int n, float* logits_all, float* logits_last);

/* Token scores (one-shot), for the NEXT vc_prefill (labels [B, T] aligned with its ids) or vc_extend (labels [B, n] aligned with its
 * tok): the loss side of the reference's forward(labels=...) (vcoder_ds_llava_llama.py:95-106) without logits leaving the device.
 * A vc_prefill splices the labels by the plan of its embeddings (vcoder_ds_llava_arch.py:176-293): a text row keeps the label of its
 * id, feature rows and the right padding of shorter rows carry -100, text the DS variant drops between <image> and <seg> drops its
 * label too, and whatever stands at a placeholder position of `labels` is ignored.  HF's shift applies: the row in front of position
 * j scores label j, position 0 of a prefill and label 0 of an extend chunk are never scored.  The final norm and the lm_head run
 * over the scored rows only, in chunks of 1024 rows, and a kernel reduces every logits row to log p(label).
 * logprobs (host, cap elements) receives [B, S] resp. [B, n] fp32: log p(label) where the spliced label is not -100, 0 elsewhere;
 * spliced_labels (host, cap elements, may be NULL) the labels as laid out.  Both must stay valid until that call returns.
 * Composes with vc_set_attention_mask, vc_set_image_counts, vc_request_hidden_states, vc_request_attentions, logits_all and
 * logits_last.  Cleared when that call returns, also when it fails; vc_generate* ignores and clears it.
 * That call refuses, with the session's cache and position unchanged (vc_extend: before anything is enqueued; vc_prefill: behind
 * its splice plan, before the decoder stack): a spliced label outside {-100} and [0, vocab) that the shift keeps (VC_ERR_INDEX:
 * torch's "Target ... is out of bounds" is an IndexError; as there, a label the splice drops is never looked at); B / T / n that do
 * not match the call, or cap smaller than the result (VC_ERR_INVALID).  For the same reason a scored vc_prefill that its plan refuses
 * on other grounds (an id outside the vocabulary, VC_ERR_UNEQUAL) keeps the loop position too, where an unscored vc_prefill has
 * already dropped it on entry; both leave the cache rows untouched.  labels == NULL cancels a pending request. */
int vc_request_token_scores(vc_model* m, const int64_t* labels, int B, int T, float* logprobs /* [B, S] or [B, n] host */,
                            int64_t* spliced_labels /* same shape, may be NULL */, size_t cap /* elements of each output buffer */);

/* Top-K alternatives of the scored positions (one-shot): accompanies a PENDING vc_request_token_scores and shares its lifetime (the
 * scored vc_prefill / vc_extend consumes both; cancelling or replacing the score request drops it).  That call fills, at every
 * position that carries a score, top_ids / top_logprobs [B, S] or [B, n] x top_k with the top_k most likely tokens of the row in front
 * of it — what the model would have said instead of the label — ordered by (log-prob descending, id ascending; ties break as the
 * greedy argmax breaks them), each as logit - logsumexp over the fp32 logits; positions without a score hold 0.0 / -1.  top_k in
 * 1 .. 32; cap = entries of each buffer (>= B * S * top_k resp. B * n * top_k, else that call fails with VC_ERR_INVALID, the
 * session's cache and position unchanged).  Without a pending score request: VC_ERR_STATE. */
int vc_request_top_logprobs(vc_model* m, int top_k, float* top_logprobs /* [B, S] or [B, n] x top_k host */,
                            int32_t* top_ids /* same shape */, size_t cap);

/* the loop steps back to position P (prefill's S <= P <= current position): cached rows >= P are dead.  Nothing is copied; the
 * prefill's hidden keys stay hidden; every precision mode.  The token the last step selected on the device is no longer valid:
 * vc_decode_step(tok = NULL) returns VC_ERR_STATE until a vc_extend or a vc_decode_step with explicit tokens has run.  K candidate
 * continuations are scored behind one prompt as K x (vc_request_token_scores, vc_extend, vc_rewind).  HF counterpart:
 * DynamicCache.crop. */
int vc_rewind(vc_model* m, int P);

/* beam search support: the KV rows of the current vc_prefill / vc_decode_step loop are permuted, row r <- old row src_rows[r] —
 * `past_key_values` reordered by beam_idx after a beam step ([HF] generation/utils.py beam_search; the reference's eval loaders
 * forward num_beams: eval/model_seg_loader.py:129-139).  It serves a host-driven beam loop (beam-sample, stopping criteria, strict
 * mode); plain beam search runs inside the device loop, vc_generate_beam below. */
int vc_reorder_cache(vc_model* m, const int32_t* src_rows, int B);

/* generate(num_beams = n) inside the device loop ([HF] GenerationMixin.beam_search + BeamSearchScorer of Transformers 4.31, as the
 * reference's eval loaders call it: batch 1, no stopping criteria).  ids [B, T] are the un-expanded rows; the engine expands every
 * sequence to n rows (b * n .. b * n + n - 1) for the encode, the splice and the prefill, then replays one captured beam step per
 * token: the linears and attention of a decode step over B * n rows, the 2 n best log-probs of every row, a selection kernel (the
 * 2 n best candidates per sequence by score, then flat index beam * V + id; BeamSearchScorer.process; hypotheses kept as
 * back-pointers), a cache permute that copies only the positions behind the prompt, and the embedding of the chosen tokens.  Scores
 * are fp32: candidate = log-prob + running beam score, hypothesis = sum / len ** length_penalty with the power taken on the host.
 * early_stopping: 0 false, 1 true, 2 "never"; len_counts_prompt != 0: a hypothesis' length counts the T prompt ids (4.31).
 * eos_ids: up to 8 ids (n_eos 0: none), pad_id < 0: none (the rows of a done sequence then emit id 0, and a result that needs
 * padding fails with VC_ERR_INVALID as HF's "`pad_token_id` has to be defined").
 * out_ids [B, max_new] host: the best hypothesis of every sequence, one EOS (eos_ids[0]) behind it where it is shorter than the
 * returned width min(longest + 1, max_new), pad_id elsewhere; out_len [B] its length; out_score [B] its score; n_steps the steps run.
 * Honours vc_set_attention_mask / vc_set_image_counts (given for the B un-expanded rows).  Runs on the session's own loop.
 * Refused before anything is touched: num_beams < 1, B * num_beams > 16, n_eos > 8 (VC_ERR_INVALID); precision mode "strict", a
 * pending vc_request_generate_logprobs or vc_request_logits_processors (VC_ERR_STATE).  More than n EOS ids among a step's 2 n best fails with VC_ERR_INVALID (HF's
 * ValueError). */
int vc_generate_beam(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                     int pixels_on_device, int num_beams, int max_new, const int32_t* eos_ids, int n_eos, int pad_id,
                     float length_penalty, int early_stopping /* 0 false, 1 true, 2 "never" */, int len_counts_prompt,
                     int32_t* out_ids /* [B, max_new] */, int32_t* out_len /* [B] */, float* out_score /* [B] */, int* n_steps);

/* greedy generate(): encode + splice + prefill + (max_new-1) hipGraph-replayed decode steps, HF semantics
 * (SURVEY.md Appendix C): eos_id < 0 disables EOS; finished rows emit pad_id; stops when all rows finished.
 * generate() always carries an attention_mask, so unequal spliced lengths fail with VC_ERR_UNEQUAL (quirk 6).
 * out_ids [B,max_new] int32 host (row-major, unused tail = pad_id); n_generated = columns produced. */
int vc_generate_greedy(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                       const float* depth, int pixels_on_device, int max_new, int eos_id, int pad_id,
                       int32_t* out_ids, int* n_generated);
/* the same with a device-side keyword stop: n_stop token sequences (stop_ids flattened,
 * stop_lens[i] ids each; at most 8 sequences of at most 8 ids).  A row is finished — later tokens are pad_id — once
 * its ids (prompt tail + generated) end with one of them; generation ends when every row is finished by EOS or a stop.
 * Batched, hipGraph-friendly form of KeywordsStoppingCriteria's id match (vcoder_llava/mm_utils.py:128-151: batch size
 * 1, evaluated on the host after every token). */
int vc_generate_greedy_stop(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                            const float* depth, int pixels_on_device, int max_new, int eos_id, int pad_id,
                            const int32_t* stop_ids, const int32_t* stop_lens, int n_stop, int32_t* out_ids,
                            int* n_generated);

/* generate() in full — what vcoder_llava/serve/cli.py:122-132 and serve/chat.py:141-151 call: greedy, or sampling on the
 * device when samp->do_sample (HF order: temperature, top-k, top-p, multinomial).  The draw is a
 * counter-based generator keyed by (seed, row of the batch, step, vocabulary index): the same seed gives the same tokens.
 * cb (may be NULL): streamer hook, called on the calling thread with the ids of steps [first_step, first_step + n_steps)
 * of every row (ids [B][n_steps] row-major) every cb_every steps — the decode loop stays hipGraph-replayed in between. */
typedef struct vc_sampling {
    int32_t do_sample;   /* 0: greedy */
    float temperature;   /* > 0 */
    int32_t top_k;       /* <= 0: off (HF's GenerationConfig default is 50) */
    float top_p;         /* (0, 1]; 1: off */
    uint64_t seed;
} vc_sampling;
typedef void (*vc_token_cb)(void* user, int first_step, int n_steps, int B, const int32_t* ids);
int vc_generate(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                int pixels_on_device, int max_new, int eos_id, int pad_id, const int32_t* stop_ids, const int32_t* stop_lens,
                int n_stop, const vc_sampling* samp, vc_token_cb cb, void* cb_user, int cb_every, int32_t* out_ids,
                int* n_generated);

/* Per-token log-probs of the NEXT vc_generate / vc_generate_greedy* call (one-shot; HF: generate(output_scores=True) +
 * compute_transition_scores(normalize_logits=True), a serving API's logprobs / top_logprobs) without logits leaving the device:
 *   token_logprobs [B, max_new]        log p(generated token)
 *   top_ids / top_logprobs [B, max_new, top_k]   the top_k most likely tokens of every step, ordered by (log-prob descending, id
 *                                      ascending — ties break as the greedy argmax breaks them); NULL iff top_k == 0
 * of the model's own next-token distribution: log_softmax of the step's fp32 logits, taken BEFORE temperature / top-k / top-p, also
 * when sampling, and before the logits processors of vc_request_logits_processors (the raw rows).  A kernel behind every selection of the loop reduces the step's logits rows; the slabs come back once, beside
 * out_ids.  A row's finishing token (its EOS, or the token that completes a stop sequence) is scored; positions behind it (the row
 * emits pad there) and columns the loop never reached hold 0.0 / 0.0 / -1.  When a greedy row's token is among its top ids, the two
 * log-probs are bit-equal.
 * The call then runs on the session's own loop (every precision mode, whatever VC_POOL says): the decode pool does not serve
 * log-probs.  The ids are those of the same call without the request.  Buffers: host, cap_rows rows ([.] or [top_k] per row), valid
 * until that call returns; cap_rows < B * max_new makes that call fail with VC_ERR_INVALID before anything is touched.  top_k
 * outside 0 .. 32 (or a missing buffer): VC_ERR_INVALID here, nothing changed.  Cleared when that call returns, also when it fails;
 * every other entry point ignores and clears it; token_logprobs == NULL cancels. */
int vc_request_generate_logprobs(vc_model* m, int top_k, float* token_logprobs /* [B, max_new] host */,
                                 float* top_logprobs /* [B, max_new, top_k] host, NULL iff top_k == 0 */,
                                 int32_t* top_ids /* same shape */, size_t cap_rows /* >= B * max_new of the call it applies to */);

/* Prompt-lookup speculative decoding for the NEXT vc_generate / vc_generate_greedy* call (one-shot; HF's prompt_lookup_num_tokens).
 * Each step of the call's loop drafts up to k ids per sequence — the ids behind the latest earlier occurrence of the sequence's last
 * max_ngram .. 1 ids in (lookup ids | prompt ids | ids generated so far) — runs the last emitted id and the drafts through the
 * decoder as k + 1 rows of ONE weight pass (a verify attention that reproduces the plain step's bits per row), and emits the model's
 * own greedy tokens for as long as the drafts agree with them.  The ids, n_generated and log-probs are those of the same call without
 * the request, in fewer steps.  lookup_ids: what the caller expects the answer to resemble (a previous turn, a class list), the B
 * sequences' ids back to back, lookup_lens[b] each; NULL / NULL: none.
 * Served on the session's own loop (whatever VC_POOL says) when the call is greedy, has no logits processors, runs in the bf16
 * precision mode, B * (k + 1) <= 32, and the score rows of k + 1 queries over the call's cache fit a CU's LDS; otherwise the call runs
 * as without the request.  vc_generate_beam ignores it.  Behind a served call the rows stand at different positions: vc_decode_step
 * and vc_extend refuse (VC_ERR_STATE) until the next prefill.  k outside 1 .. 7, max_ngram outside 1 .. 4, lengths outside
 * 0 .. max_position_embeddings or more than 16 sequences: VC_ERR_INVALID here, nothing changed; a B other than the call's makes that
 * call fail with VC_ERR_INVALID.  Cleared when that call returns, also when it fails; k == 0 cancels. */
int vc_request_speculation(vc_model* m, int k, int max_ngram, const int32_t* lookup_ids, const int32_t* lookup_lens, int B);
/* The selections the pending vc_request_speculation is served for (one-shot: it travels with that request, is cleared with it, and
 * VC_ERR_STATE without one).  any == 0, the default: greedy calls without logits processors, as above.  any != 0: sampled calls
 * (temperature / top-k / top-p, any seed) and calls with a vc_request_logits_processors set are served too, greedy ones through the
 * same step.  The device sampler is a Gumbel-max keyed by (seed, generated index, vocabulary id): the verify step samples query row j
 * with the key of the token it would become and accepts a draft while it equals the token sampled in front of it, and it processes
 * row j over the row's history plus the j drafts in front of it — so ids, n_generated and log-probs (those of the raw rows) are
 * still those of the same call, same seed, without the request: no acceptance probability is involved.  Opt-in because a served call
 * leaves the decode pool and closes the session's loop, which a sampled caller has to ask for.  The other conditions stand: the bf16
 * precision mode, B * (k + 1) <= 32, the LDS bound; vc_generate_beam and a served vc_request_fanout ignore the request. */
int vc_request_speculation_selection(vc_model* m, int any);
/* Per-sequence counters of the last vc_generate* call of this session: out[b] = {verify steps, tokens they emitted, drafts proposed,
 * drafts accepted}.  VC_ERR_STATE when that call did not speculate. */
int vc_last_speculation(vc_model* m, int32_t* out /* [B][4] */, int B);

/* num_return_sequences for the NEXT vc_generate call (one-shot): every prompt yields n sequences.  That call takes B prompts (ids and
 * pixels of B samples) and returns out_ids [B n, max_new], rows b n + j; its log-prob buffers and the callback's columns are B n rows
 * wide.  The result is, bit for bit, that of the same call on the prompts repeated n times (row r seeds its sampler with its own
 * index).  Served — one prefill over the B prompts, whose keys and values every step of the B n rows reads once per prompt with the
 * fan-out attention — on the session's own loop (whatever VC_POOL says) in the bf16 precision mode with head dim 128 or 64, a bf16
 * or e4m3 cache, 2 <= n <= 8, n score rows over max_position_embeddings keys within a CU's LDS, and a prefill whose bits do not
 * depend on the rows sharing its launch — vc_model_set_batch_invariant(1), or shapes at which no GEMM of the repeated call's prefill
 * has more than one round of tiles (else the repeated call gives identical prompts different bits and no shared prefix equals it);
 * every weight format, log-probs and logits processors included.  Otherwise the engine repeats the prompts, pixels, image counts and mask rows n times and runs the call
 * as it would run B n prompts.  Behind a served call a cache row no longer holds one sequence: vc_decode_step and vc_extend refuse
 * (VC_ERR_STATE) until the next prefill.  B n > 16 makes that call fail with VC_ERR_INVALID.  |n| above 16: VC_ERR_INVALID here,
 * nothing changed.  n < -1: |n| sequences per prompt, never served (the repeated prompts: the reference of the served form).  Cleared
 * when that call returns, also when it fails; -1 .. 1 cancels.  vc_generate_beam ignores it. */
int vc_request_fanout(vc_model* m, int n);
/* What the last vc_generate of this session made of a fan-out request: out = {n, shared (1: served; 0: the prompts were repeated),
 * prompt rows the prefill ran over (B when served, B n otherwise)}.  VC_ERR_STATE when that call had no request. */
int vc_last_fanout(vc_model* m, int32_t* out /* [3] */);

/* Classifier-free guidance of the NEXT vc_generate or vc_prefill call (one-shot; HF's generate(guidance_scale=, negative_prompt_ids=),
 * UnbatchedClassifierFreeGuidanceLogitsProcessor).  neg_ids [B, Tn] int64: the negative prompt of every sequence of that call —
 * rectangular, unpadded, placeholders allowed when neg_img (and neg_seg / neg_depth as the variant takes them) bring one image per
 * sample, as the pixels of vc_generate; copied here.  The pixel pointers are borrowed: they must stay valid until that call returns.
 * Every step scores the next token behind the prompt (raw row c) and behind the negative prompt (raw row u), both followed by the ids
 * generated so far, and replaces c by
 *     out = scale * (lc - lu) + lu,   lc = (c - max c) - log(sum(exp(c - max c))),  lu likewise      (fp32, no fused multiply-add)
 * as the input of everything behind it: the logits processors (the repetition penalty's sign test runs on these log-domain values,
 * as in HF, where guidance is the first processor), the token automaton, the warpers, the greedy or sampled selection.  Log-probs
 * (vc_request_generate_logprobs) stay those of the raw row c.  EOS, stop sequences and max_new are decided on the conditional row.
 * A served vc_generate runs on the session's own loop (whatever VC_POOL says) over 2 B rows in ONE weight pass per step — rows
 * 0 .. B - 1 the call's sequences, rows B .. 2 B - 1 their followers behind the negative prompts, which take over every chosen token —
 * after two prefills of B rows each (each prompt gets the bits a call of its own gives it); out_ids, the log-prob buffers and the
 * callback's columns stay B rows wide.  A vc_generate is served in the bf16 precision mode (VC_ERR_STATE otherwise), every weight format, bf16 and
 * e4m3 caches, greedy and sampled, with logits processors, a token automaton, log-probs, EOS, stop sequences and a callback; a pending
 * vc_request_speculation is not served beside it, a pending vc_request_fanout makes the call fail (VC_ERR_STATE), vc_generate_beam
 * refuses (VC_ERR_STATE).  The cache holds max(spliced prompt, spliced negative prompt) + max_new positions (VC_ERR_INVALID beyond
 * max_position_embeddings).  Behind a served vc_generate the rows stand at different positions: vc_decode_step and vc_extend refuse
 * (VC_ERR_STATE) until the next prefill.
 * vc_prefill with a pending request builds the same state for a host loop, in EVERY precision mode (bf16, strict, split — the strict
 * step then reads every row's own position); has_attention_mask applies to both prompts (the unequal-length quirk); logits_last
 * receives [2 B, V] (the prompts' rows, then the negative prompts'), *S_out the prompts' spliced length, and vc_decode_step then takes 2 B tokens and returns 2 B rows, every row
 * advancing its own position (tok == NULL, vc_extend, vc_rewind and vc_reorder_cache refuse; no labels / all-row logits / hidden
 * states / attentions beside it).  The combination itself is then the host's (logits_processors.apply_guidance).
 * A non-finite scale, B < 1, 2 B > 16 or Tn < 1: VC_ERR_INVALID, nothing changed; B other than that call's batch makes the call fail.
 * neg_ids == NULL cancels.  Cleared when that call returns, also when it fails. */
int vc_request_guidance(vc_model* m, float scale, const int64_t* neg_ids, int B, int Tn, const float* neg_img, const float* neg_seg,
                        const float* neg_depth, int pixels_on_device);
/* What the last vc_generate / vc_prefill of this session made of a guidance request: out = {1 (served), B, spliced length of the
 * prompts, spliced length of the negative prompts}.  VC_ERR_STATE when that call had no request. */
int vc_last_guidance(vc_model* m, int32_t* out /* [4] */);

/* The further warpers of the NEXT vc_generate call (one-shot): HF's MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and
 * EtaLogitsWarper with min_tokens_to_keep = 1, applied on the device behind those of vc_sampling, in HF's order:
 *     temperature -> top-k -> top-p -> min-p -> typical -> epsilon -> eta -> draw
 * Every warper sees the row with what those in front of it removed at -inf: its softmax and its entropy H are taken over the survivors.
 *   min_p           p < min_p * max p is removed (the maximum always stays).  [0, 1]; 0: off
 *   typical_p       s_i = |-log p_i - H|; in ascending order of s the first tokens whose cumulative probability reaches typical_p stay,
 *                   equal s together.  > 0; >= 1: off
 *   epsilon_cutoff  p < epsilon_cutoff is removed unless the score equals the maximum.  [0, 1); 0: off
 *   eta_cutoff      p < min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)) is removed unless the score equals the maximum.  [0, 1); 0: off
 * The values travel in the rows' records, so the request neither moves a call to another loop (a sampled call of the decode pool runs
 * there, beside rows with other settings) nor changes a captured step; logits processors, a token automaton, guidance, log-probs, a
 * fan-out and speculation with the "any" selection select through the same code and combine freely.  A greedy call (samp NULL or
 * do_sample 0) applies none of them, as HF does.  With all four off the call takes the path and returns the bits it would without
 * the request.  A value outside its range: VC_ERR_INVALID, nothing changed.  Cleared when the next vc_generate returns, also when it
 * fails; vc_prefill, vc_generate_beam and the scoring calls ignore and clear it. */
int vc_request_sampling_warpers(vc_model* m, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff);

/* Logits processors of the NEXT vc_generate / vc_generate_greedy* call (one-shot), applied on the device in front of every selection
 * of the loop, in HF 4.31's order (generation/logits_process.py):
 *   repetition_penalty p   RepetitionPenaltyLogitsProcessor: every id t of the row's history gets raw[t] < 0 ? raw[t] * p : raw[t] / p
 *                          (IEEE fp32).  > 0 and finite; 1.0: off
 *   no_repeat_ngram_size n NoRepeatNGramLogitsProcessor: -inf for every token that would complete an n-gram the history already
 *                          holds; n = 1 bans every history id; 0: off
 *   bad words              NoBadWordsLogitsProcessor: at most 32 sequences of 1 .. 8 ids (bad_words_ids flattened, bad_words_lens[i]
 *                          ids each): a one-id sequence is always -inf, a longer one bans its last id while the history ends
 *                          with the ids in front of it
 *   min_new_tokens m       MinNewTokensLengthLogitsProcessor: while fewer than m tokens are generated, the call's eos_id and the
 *                          eos_extra ids (the further ids of an EOS list, at most 8) are -inf; stop sequences are unaffected.
 *                          HF's min_length is max(m, min_length - T) on the caller's side (HF counts the un-spliced input_ids)
 * The history of a row is the caller's ids [T] (image placeholders and all) followed by the ids generated so far.  History ids
 * outside [0, vocab) are skipped — HF itself would raise an index error on the image placeholders there.  A token that is both
 * penalised and banned is -inf.
 * The call then runs on the session's own loop (every precision mode, whatever VC_POOL says; strict mode enqueues its steps
 * eagerly): a kernel in front of every selection writes a processed copy of the step's logits rows, which the selection — greedy or
 * sampled — reads; the parameters travel in the rows' records, so one captured step serves every setting.  Per-token log-probs
 * (vc_request_generate_logprobs) of such a call stay those of the RAW rows: the model's own distribution, before processors as well
 * as before temperature / top-k / top-p.
 * Refused with VC_ERR_INVALID, nothing changed: a penalty that is not above 0 or not finite, a negative n or m, more than 32
 * sequences, a sequence that is empty or longer than 8 ids, more than 8 eos_extra ids.  The struct and its arrays are copied here.
 * Cleared when that call returns, also when it fails; every other entry point ignores and clears it — except vc_generate_beam,
 * which refuses to run with VC_ERR_STATE while one is pending (and clears it); p == NULL cancels. */
typedef struct vc_logits_processors {
    float repetition_penalty;
    int32_t no_repeat_ngram_size;
    int32_t min_new_tokens;
    int32_t n_bad_words;
    const int32_t* bad_words_ids;
    const int32_t* bad_words_lens;
    int32_t n_eos_extra;
    const int32_t* eos_extra;
} vc_logits_processors;
int vc_request_logits_processors(vc_model* m, const vc_logits_processors* p);

/* Constrained decoding of the NEXT vc_generate / vc_generate_greedy* call (one-shot): a deterministic automaton over token ids.
 * State s owns the edges state_off[s] .. state_off[s + 1] (CSR); edge_tok is ascending and unique within a state, edge_next the state
 * behind an edge; default_next[s] >= 0: every id without an edge is allowed too and leads there (free text), -1: only the ids with
 * an edge are allowed.  State 0 is the start state, -1 the dead state (nothing is allowed).  A row starts in state 0 at its first
 * generated token; in front of every selection the ids its state does not allow are set to -inf in the processed copy of the
 * step's logits row, behind the processors of vc_request_logits_processors (HF 4.31's place of PrefixConstrainedLogitsProcessor);
 * edge ids outside [0, vocab) are ignored; a finished row keeps emitting pad.  The call runs on the session's own loop (every
 * precision mode, greedy or sampled, with or without processors, log-probs — which stay those of the RAW rows — EOS ids, stop
 * sequences, a callback, vc_request_fanout in both forms); a pending vc_request_speculation is not served beside it (the call
 * runs as without it).
 * Refused with VC_ERR_INVALID, nothing changed: more than 65536 states or 1 << 20 edges, a missing table, a state_off that does not
 * rise from 0 to n_edges, edge ids that are not ascending and unique within a state, a target outside [-1, n_states), a state
 * reachable from 0 that allows no token.  The tables are copied here and uploaded when the call is armed.  Cleared when that call
 * returns, also when it fails; every other entry point ignores and clears it — except vc_generate_beam, which refuses to run with
 * VC_ERR_STATE while one is pending (and clears it); a == NULL cancels. */
#define VC_MAX_AUTOMATON_STATES 65536
#define VC_MAX_AUTOMATON_EDGES (1 << 20)
typedef struct vc_token_automaton {
    int32_t n_states;
    int32_t n_edges;
    const int32_t* state_off;     /* [n_states + 1] */
    const int32_t* edge_tok;      /* [n_edges] */
    const int32_t* edge_next;     /* [n_edges] */
    const int32_t* default_next;  /* [n_states] */
} vc_token_automaton;
int vc_request_constraint(vc_model* m, const vc_token_automaton* a);

/* spliced sequence length (text rows + feature rows) of the last vc_generate_greedy* call: lets a caller that splits a large
 * batch into replica-sized pieces reproduce the reference's whole-batch behaviour for unequal lengths (quirk 6) */
int vc_last_spliced_len(vc_model* m);

/* ---- next row §8(f)2: image preprocessing on the device ------------------------------------------------------------
 * process_images() of vcoder_llava/mm_utils.py:28-40 for ONE image: expand2square(mean colour) when pad_to_square,
 * PIL-exact bicubic resize (shortest edge -> S) + center crop, rescale 1/255, (x-mean)/std, HWC->CHW.
 * rgb: uint8 [h,w,3] on the host; out: fp32 [3,S,S] (device pointer when out_on_device, else host). */
int vc_preprocess_image(vc_model* m, const uint8_t* rgb, int h, int w, int pad_to_square, const float* mean,
                        const float* stdv, float* out, int out_on_device);

/* ---- multi-GPU: the one exchange of the data-parallel path ------------------------------------------
 * Image batches shard over the GPUs of a node with no collective on the data path; the only exchange is an all-gather of
 * the generated token ids (the reference: one answers file per GPU process + `cat`, scripts/v1_5/eval/cost_depth.sh:10-34).
 * RCCL (ncclAllGather over xGMI) is called directly on the context's stream; librccl is bound with dlopen at first use.
 * Rank 0 obtains the 128-byte RCCL unique id and distributes it through any side channel; world 1 needs no id and no RCCL. */
typedef struct vc_comm vc_comm;
int vc_comm_unique_id(vc_ctx* ctx, void* out128);
int vc_comm_create(vc_ctx* ctx, int rank, int world, const void* unique_id128, vc_comm** out);
/* 1 when the communicator's gathers run through RCCL: world > 1, or a SINGLE rank created with VC_COMM_FORCE_RCCL=1 in the
 * environment (a one-rank ncclCommInitRank + ncclAllGather on the stream: the multi-GPU code path on a one-GPU box) */
int vc_comm_uses_rccl(vc_comm* comm);
/* global[r * n + i] = rank r's local[i]; host buffers (n int32 per rank) */
int vc_allgather_tokens(vc_comm* comm, const int32_t* local, int n, int32_t* global);
void vc_comm_destroy(vc_comm* comm);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------------- */
/* times `reps` sweeps of every decode GEMV launch of one step (4 per layer + lm_head) over B <= 32 rows with HIP events on
 * the model's stream; returns launches per sweep, average microseconds per launch, algorithmic weight bytes per launch */
int vc_profile_decode_gemv(vc_model* m, int B, int reps, int* launches, double* avg_us, double* avg_bytes);
/* cumulative number of pooled decode steps launched over 8 / 16 / 24 / 32 rows since the pool of m's root model was created
 * (zeros without a pool): weights the per-row-count kernel timings by what a timed run actually executed */
int vc_pool_step_counts(vc_model* m, unsigned long long* counts4);
/* In-situ timing of the pool's decode-step kernels (bench.py `roofline`: the dominant kernel AS IT RAN in the timed region, beside
 * whatever the other sessions had on the GPU — not a replay).  on != 0: the pool's step graphs are (re)captured with one timing slot
 * per launch; the first thread of every workgroup writes its own {start, end} on the device's constant-rate wall clock (plain
 * stores, no atomics), and one small launch per step folds the slots into per-(span, kind) sums of (latest end - earliest start).  Takes effect when the pool is next (re)built, i.e. while
 * no generate() is in flight.  bf16 path only.  No reference counterpart (the reference has no timing code). */
int vc_pool_profile(vc_model* m, int on);
/* Pool scheduling: on = 1 (default) the pool does not step while a generate() call that already holds rows is still prefilling —
 * it waits for that request to join instead of running a step beside the prefill's GEMMs (2-7x a step's time) that the joiner
 * would need again anyway; on = 0 steps whatever rows are active (lower inter-token latency for the calls in flight, lower
 * throughput).  No reference counterpart (the reference runs one generate() at a time). */
int vc_pool_set_hold(vc_model* m, int on);
/* Rows of the shared decode pool: 32 (default) or 64 (round-6 measurement: two 32-row weight passes per step).  Takes effect when the
 * pool is next built (idle).  64 rows: bf16 step only, no in-situ timing. */
int vc_pool_set_rows(vc_model* m, int rows);
/* sums since the last reset, each [4 spans: 8 / 16 / 24 / 32 rows][6 kinds: qkv, decode attention, o_proj, gate/up, down, lm_head]:
 * exec_us = earliest workgroup start -> latest workgroup end of the launches; period_us = latest end of the previous launch of the
 * step -> latest end of this one (dispatch, drain and inter-kernel gap included: what the step's dependency chain pays per launch;
 * rocprofv3's per-kernel duration lies between the two); launches.  reset != 0 zeroes them.  The pool must be idle. */
int vc_pool_profile_read(vc_model* m, double* exec_us, double* period_us, unsigned long long* launches, int reset);
/* the same for the decode attention launches of one step (one per layer) over B rows at context ~ctx: launches per sweep,
 * average microseconds per launch, algorithmic KV bytes per launch (K and V rows of every key, bf16) */
int vc_profile_decode_attention(vc_model* m, int B, int ctx, int reps, int* launches, double* avg_us, double* avg_bytes);
/* wall-clock split of the last vc_generate_greedy in ms (HIP events): encode, prefill, decode */
int vc_last_timings(vc_model* m, float* encode_ms, float* prefill_ms, float* decode_ms);

#ifdef __cplusplus
}
#endif
#endif /* VCODER_HIP_H */
