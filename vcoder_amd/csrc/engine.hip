// engine.hip — host-side engine + C ABI (include/vcoder_hip.h) of the MI355X-native VCoder hot path.
//
// Owns: weights (HF key -> fused / interleaved / MFMA-packed device layouts), the ViT and LLM workspaces,
// the KV cache (K key-major, V transposed), rope tables, the splice planner, and the hipGraph of one
// decode step.  Replaces L0-L2 (+ forward/generate of L3) of the reference:
//   CLIPVisionTower.forward            vcoder_llava/model/multimodal_encoder/clip_encoder.py:39-51
//   encode_*                            vcoder_llava/model/vcoder_ds_llava_arch.py:106-124
//   prepare_inputs_labels_for_multimodal  vcoder_ds_llava_arch.py:126-314, vcoder_llava_arch.py:146-296, llava_arch.py:99-199
//   ...ForCausalLM.forward              vcoder_llava/model/language_model/vcoder_ds_llava_llama.py:57-118
//   HF greedy loop                      SURVEY.md Appendix C
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vcoder_hip.h"
#include "kernels.h"

using namespace vc;

#define VC_API extern "C" __attribute__((visibility("default")))

static const int IMAGE_TOKEN_INDEX = -200;  // vcoder_llava/constants.py:5
static const int SEG_TOKEN_INDEX = -300;    // constants.py:8
static const int DEPTH_TOKEN_INDEX = -400;  // constants.py:11
static const int IGNORE_INDEX = -100;       // constants.py:4
static const int VC_MAX_ROWS = 16;          // sequences one prefill / one session loop handles
// The prefill's RMSNorm output rows are padded by 64 elements: with both GEMM operands at a row stride of exactly 2^13
// bytes (K = 4096 bf16) the 9728 x 12288 QKV GEMM of the 7b model ran 19 % slower (915 vs 770 us; address aliasing
// between the concurrently fetched panels — tools/experiments/gemm_rounds.py); no other shape cares.
static const int XN_PAD = 64;
static const int VC_POOL_ROWS = 32;         // rows of the shared decode pool (two MFMA token-slot groups = one weight pass per step)
static const int VC_POOL_ROWS_MAX = 64;     // vc_pool_set_rows(64): a pool whose step takes two 32-row weight passes (measurement)

#include "engine_ctx.h"

namespace {

struct Fail {
    int code;
    std::string msg;
};
#define HIPCHK(x)                                                                                       \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess)                                                                           \
            throw Fail{VC_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)};                     \
    } while (0)
#define REQUIRE(cond, code, ...)                                                                        \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            char b_[512];                                                                               \
            snprintf(b_, sizeof b_, __VA_ARGS__);                                                       \
            throw Fail{code, b_};                                                                       \
        }                                                                                               \
    } while (0)

inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

// stream of the session whose C-ABI call is running on this host thread (set by USE_DEVICE); zero-fills of freshly
// allocated buffers are enqueued on it — never on the legacy NULL stream, which would implicitly synchronise with (and
// invalidate the graph capture of) other sessions' streams
thread_local hipStream_t t_stream = nullptr;

// Every session and the decode pool get their own non-blocking stream.  (Rounds 3-4 measured CU masks and queue priorities for
// them — disjoint CU ranges for the MFMA-bound and the HBM-bound phase, high / low priority queues: all negative,
// profiles/r03_a_cu_mask_experiment.md, r03_q_stream_priority_and_inflight.md — and the knobs were removed in round 5.)
hipStream_t make_stream() {
    hipStream_t st = nullptr;
    // non-blocking: no implicit synchronisation with the legacy NULL stream (torch's default stream, other sessions)
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    return st;
}

struct Buf {  // grow-only device buffer
    void* p = nullptr;
    size_t cap = 0;
    void ensure(size_t bytes, bool zero = false) {
        if (bytes <= cap) return;
        if (p) HIPCHK(hipFree(p));
        p = nullptr;
        cap = 0;
        HIPCHK(hipMalloc(&p, rup(bytes, 256)));
        cap = rup(bytes, 256);
        if (zero) {
            HIPCHK(hipMemsetAsync(p, 0, cap, t_stream));
            HIPCHK(hipStreamSynchronize(t_stream));
        }
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct VitLayer {
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_b, *out_b, *fc1_b, *fc2_b;
    bf16_t *qkv_w, *out_w, *fc1_w, *fc2_w;
};
struct LlmLayer {
    float *in_norm, *post_norm;
    bf16_t *qkv_w, *o_w, *gate_tmp, *up_tmp, *gu_w, *down_w;  // row-major (prefill GEMM)
    bf16_t *qkv_p, *o_p, *gu_p, *down_p;                      // MFMA-fragment packed (decode GEMV); e4m3 bytes if W8A16
    float *qkv_s = nullptr, *o_s = nullptr, *gu_s = nullptr, *down_s = nullptr;  // W8A16 per-output-row scales
    uint8_t *qkv_q = nullptr, *o_q = nullptr, *gu_q = nullptr, *down_q = nullptr;  // weight format 2: e4m3 bytes, row-major
};
struct Projector {
    int depth = 0;
    std::vector<bf16_t*> w;
    std::vector<float*> b;
};

// Everything one decode step touches besides the weights: the buffers of a session's own loop or of the shared pool.
struct LoopView {
    hipStream_t st;
    bf16_t *kc, *vc;   // [L][capR][H][capS][hd]: K and V, both key-major (fp32 elements when es == 4)
    int es;            // bytes per cache element: 2 (bf16); precision mode "split": 3 (fp24) or 4 (fp32)
    int split_G;       // 0: bf16 decode step.  G = 8 / 16: split decode step — xg_dec / attn_dec / h_dec hold stacked groups of
                       // G bf16 hi rows + G lo rows (row r -> group r / G), qkv_dec is fp32
    int capR, capS;
    int* rows;         // RowState records
    const uint8_t* kmask;  // keys hidden from the rows' decode steps ([rows][kmask_stride] bytes, 0 = hidden), or nullptr
    int kmask_stride;
    int fan_n;             // > 1: a fan-out step (vc_request_fanout) — rows g n .. g n + n - 1 share the prompt keys of cache row g
    float* x_dec;
    bf16_t *xg_dec, *qkv_dec, *attn_dec, *h_dec;
    float* logits;
    int *next_tok, *out_ids;
    float *ssq, *sk_scratch;
    unsigned* sk_counters;
    // in-situ timing (vc_pool_profile): slot s of the step = stamps + s * STAMP_SLOT_WORDS; *stamp_next = the next free slot while
    // the step is being enqueued; prof_acc = this span's accumulators.  All nullptr when off.
    unsigned* stamps;
    int* stamp_next;
    unsigned long long* prof_acc;
    unsigned* stamp_scratch;
    // per-token log-probs of a generate() call (vc_request_generate_logprobs): slabs laid out like out_ids — the chosen token's
    // log-prob [slots], the lp_k most likely tokens [slots, lp_k].  lp_tok == nullptr (every view but the one such a call makes for
    // itself): the step has no log-prob launch.
    float *lp_tok, *lp_top;
    int* lp_ids;
    int lp_k;              // (padding follows, as behind kmask_stride)
    // logits processors of a generate() call (vc_request_logits_processors): the call's prompt ids and bad-word table, and the
    // processed rows the selection then reads.  proc_logits == nullptr (every view but the one such a call makes for itself): no
    // processor launch, the selection reads the raw rows.
    const int *proc_prompt, *proc_bad;
    float* proc_logits;
    const int* fan_P;      // fan-out step: the prompt length of every group (device ints), else nullptr
    // the token automaton of a generate() call (vc_request_constraint): its tables on the device (LogitsProcessArgs::cn_*); the rows'
    // switch and state travel in their records (RS_CN_*).  nullptr / 0 (every view but the one such a call makes for itself): the
    // processor launch, if the step holds one, has no fourth phase
    const int *cn_state_off, *cn_edge_tok, *cn_edge_next, *cn_default_next;
    int cn_states;         // (padding follows)
    // classifier-free guidance of a generate() call (vc_request_guidance): the step runs over 2 B rows — B conditional rows and their
    // B followers behind them — and its selection tail combines each pair of raw rows into gd_logits [B, V] (gd_scalars [B, 4]: the
    // combine kernel's reduction scalars), selects for the B conditional rows and lets the followers take over the chosen tokens.
    // nullptr (every view but the one such a call makes for itself): a plain tail over all rows of the step
    float *gd_logits, *gd_scalars;
};
inline bool operator==(const LoopView& a, const LoopView& b) {
    static_assert(sizeof(LoopView) == 304, "LoopView changed: compare the new member here");
    return a.st == b.st && a.kc == b.kc && a.vc == b.vc && a.es == b.es && a.split_G == b.split_G && a.capR == b.capR &&
           a.capS == b.capS && a.rows == b.rows && a.kmask == b.kmask && a.kmask_stride == b.kmask_stride && a.x_dec == b.x_dec &&
           a.xg_dec == b.xg_dec && a.qkv_dec == b.qkv_dec && a.attn_dec == b.attn_dec && a.h_dec == b.h_dec && a.logits == b.logits &&
           a.next_tok == b.next_tok && a.out_ids == b.out_ids && a.ssq == b.ssq && a.sk_scratch == b.sk_scratch &&
           a.sk_counters == b.sk_counters && a.stamps == b.stamps && a.stamp_next == b.stamp_next && a.prof_acc == b.prof_acc &&
           a.stamp_scratch == b.stamp_scratch && a.lp_tok == b.lp_tok && a.lp_top == b.lp_top && a.lp_ids == b.lp_ids &&
           a.lp_k == b.lp_k && a.proc_prompt == b.proc_prompt && a.proc_bad == b.proc_bad && a.proc_logits == b.proc_logits && a.fan_n == b.fan_n && a.fan_P == b.fan_P &&
           a.cn_state_off == b.cn_state_off && a.cn_edge_tok == b.cn_edge_tok && a.cn_edge_next == b.cn_edge_next &&
           a.cn_default_next == b.cn_default_next && a.cn_states == b.cn_states && a.gd_logits == b.gd_logits &&
           a.gd_scalars == b.gd_scalars;
}

// The buffers of the device beam loop (vc_generate_beam): the fixed-size part carved from m->bm_state, the tables from m->bm_tab /
// m->bm_den, the staging of the tail permute (ensure_beam sizes them; beam_view fills this in).
struct BeamLoop {
    float* cand_lp;   // [16, 32]
    int* cand_id;
    float* score;     // [16]
    int *perm, *start, *seq, *hyp, *params, *flags;
    int *tok_tab, *parent_tab;   // [cap_new][R]
    float *hyp_den, *done_den;   // [cap_new + 1]
    void* tmp;                   // the tail permute's staging: 2 R heads spans of span_cap bytes
    size_t span_cap;             // bytes one (row, head) of the staging holds: the cache rows of cap_new positions
    int B, n, cap_new;           // (4 bytes of padding follow: a new 4-byte member here keeps sizeof — extend operator== yourself)
};
inline bool operator==(const BeamLoop& a, const BeamLoop& b) {
    static_assert(sizeof(BeamLoop) == 136, "BeamLoop changed: compare the new member here");
    return a.cand_lp == b.cand_lp && a.cand_id == b.cand_id && a.score == b.score && a.perm == b.perm && a.start == b.start &&
           a.seq == b.seq && a.hyp == b.hyp && a.params == b.params && a.flags == b.flags && a.tok_tab == b.tok_tab &&
           a.parent_tab == b.parent_tab && a.hyp_den == b.hyp_den && a.done_den == b.done_den && a.tmp == b.tmp &&
           a.span_cap == b.span_cap && a.B == b.B && a.n == b.n && a.cap_new == b.cap_new;
}

// What a captured decode step of a session was enqueued from, and so the condition under which its hipGraphExec_t may be replayed:
// a step is replayed iff the key of the step the caller asks for equals the key it was captured from (step_graph).
//
// Audit of what enqueue_decode_step / enqueue_selection / enqueue_beam_tail hand to a launch.  Every value is
//   (a) fixed after vc_model_finalize: the weights, their scales and lo planes (lo_of), embed, the norm weights, the RoPE tables, the
//       config (hidden, ffn, heads, layers, vocab, rms_eps, max_positions), hd, npart, the weight format, sk_floats / sk_counters_n
//       (functions of the config), the RS_* / B?_* record layouts, the `advance` constant of a captured step (3);
//   (b) a member of the key: every LoopView member (the stream, the caches with es / capR / capS, the RowState records, the key mask
//       pointer — nullptr for an unmasked step — and its stride, the per-step buffers, out_ids, the split-K scratch and counters, the
//       timing pointers, the log-prob slabs with lp_k, the processor buffers, the token automaton's tables with their state
//       count), nrows, and for a beam step every BeamLoop member (the
//       state pointers, the tables, the staging with its span capacity, B, n, cap_new); or
//   (c) derived from (a) and (b) alone: the per-layer cache addresses (kc / vc, capR, capS, es, heads, hd), the attention's cache
//       format (split_G, es), the GEMV pass layout (split_G, nrows), which launches the tail holds (lp_tok, proc_logits, has_beam),
//       the beam rows R = B n.
// Two things a step bakes in are none of these and keep an explicit drop_graph:
//   - m->precision, which select_args and the beam tail read for the embedding's lo plane: vc_model_set_precision drops the steps
//     (the strict mode, 1, never captures one);
//   - the model's life: vc_model_destroy.
// Sizes matter as much as addresses: a buffer freed and allocated again may come back at the same address (B 2 -> 3 keeps the
// 16-row-padded step buffers and re-allocates the KV cache), so every capacity a launch bakes in — capR, capS, es, cap_new and the
// span capacity, lp_k — is a key member as well.  Capacities no launch bakes in are not: the rows' slots in out_ids and the slabs
// come from RS_OUT_OFF of the records, so out_stride is not part of a step.
// Baked in and NOT keyed, as before: the process-wide kernel-selection knobs of kernel_api.cpp that a decode step's launchers read —
// vck_set_gemv_variant and vck_set_gemv_wide (the third, vck_set_gemm_force_8phase, concerns the prefill GEMMs only) — and the
// VC_SPLIT_KV environment switch (read once per process; it shows in es anyway).  A step captured before one of the knobs is turned stays
// on the kernels it was captured with.
// A verify step of prompt-lookup speculation (STEP_SPEC) bakes in, beside its view (whose per-step buffers hold B * Q rows) and
// nrows = B * Q: the draft's token rows, query counts, counters, the lookup / prompt id stores with their strides (the lengths are
// read on the device), the log-prob scratch with its width, and B, Q, the n-gram size.  A step of the wider scope
// (vc_request_speculation_selection) additionally holds the spec_select launch — `sel` — the verify form of the processors when the
// view carries their buffers (proc_prompt / proc_bad are view members) — `proc_out`, the B * Q processed rows — and, with log-probs,
// the chosen-token scratch `s_chosen`; nullptr each in a step that lacks the launch, so the three say which launches it holds.
// A fan-out step (STEP_FAN; vc_request_fanout) is a plain step over R = B n rows whose attention is launch_attention_fanout: beside
// the view's members it bakes in the fan-out width (fan_n: the group of a row, the prefix row g of group g, the kernel's
// instantiation) and the address of the groups' prompt lengths (fan_P; the lengths themselves are read on the device) — both are
// LoopView members, so (b) covers them: another n, or another B at the same n (nrows), re-captures; the same (B, n) replays.  The
// cache capacity in rows (capR) bounds the rows the kernel touches and is a member already.
// A guided step (STEP_GUIDE; vc_request_guidance) is a plain step over nrows = 2 B rows whose selection tail holds the combine and the
// follow launch: beside the view's members it bakes in the guided rows and the scalars' address (gd_logits / gd_scalars, LoopView
// members: non-null says the tail is the guided one) and B = nrows / 2.  The scale is read from the records on the device.
struct SpecLoop {
    int *tok, *nq, *counters;
    const int *lookup, *lookup_len, *prompt, *prompt_len;
    float* s_lp;
    int* s_ids;
    int* sel;           // [B * Q] the rows' selections (launch_spec_select), or nullptr: the accept kernel takes the argmax itself
    float* s_chosen;    // [B * Q] log-prob of sel[..] (log-probs with sel), else nullptr
    float* proc_out;    // [B * Q, V] the processed rows spec_select reads (sel with a processor set), else nullptr
    int lookup_stride, prompt_stride, s_k, B, Q, ngram;
};
inline bool operator==(const SpecLoop& a, const SpecLoop& b) {
    static_assert(sizeof(SpecLoop) == 120, "SpecLoop changed: compare the new member here");
    return a.sel == b.sel && a.s_chosen == b.s_chosen && a.proc_out == b.proc_out && a.tok == b.tok && a.nq == b.nq && a.counters == b.counters && a.lookup == b.lookup && a.lookup_len == b.lookup_len &&
           a.prompt == b.prompt && a.prompt_len == b.prompt_len && a.s_lp == b.s_lp && a.s_ids == b.s_ids &&
           a.lookup_stride == b.lookup_stride && a.prompt_stride == b.prompt_stride && a.s_k == b.s_k && a.B == b.B && a.Q == b.Q &&
           a.ngram == b.ngram;
}
struct StepKey {
    LoopView view;
    int nrows;
    bool has_beam;
    BeamLoop beam;   // zeroes without one
    SpecLoop spec;   // zeroes without one (Q == 0)
};
inline bool operator==(const StepKey& a, const StepKey& b) {
    static_assert(sizeof(StepKey) == sizeof(LoopView) + 8 + sizeof(BeamLoop) + sizeof(SpecLoop), "StepKey changed: compare the new member here");
    return a.view == b.view && a.nrows == b.nrows && a.has_beam == b.has_beam && a.beam == b.beam && a.spec == b.spec;
}
// one captured step per kind, so that a plain vc_decode_step behind a log-prob, a beam or a speculated call replays without a re-capture
enum StepKind {
    STEP_PLAIN = 0,
    STEP_CALL = 1,   // a generate() call's own: log-probs and / or processors
    STEP_BEAM = 2,
    STEP_SPEC = 3,   // the verify step of prompt-lookup speculation
    STEP_FAN = 4,    // the step of a fan-out call (num_return_sequences): the fan-out attention, with or without log-probs / processors
    STEP_GUIDE = 5,  // the step of a guided call (guidance_scale): 2 B rows, the guided selection tail, with or without log-probs / processors
    STEP_KINDS = 6
};
struct StepGraph {
    StepKey key{};
    hipGraphExec_t exec = nullptr;
};

}  // namespace

struct vc_model {
    vc_ctx* ctx;
    vc_model_cfg c;
    hipStream_t st;
    bool finalized = false;
    bool owns_weights = true;
    int precision = 0;  // 0: bf16 MFMA fast path; 1: strict fp32 path (strict.hip); 2: split — fp32 activations in HBM,
                        // every MFMA operand as bf16 hi + lo fragments on the fast kernels
    int kv_es = 2;      // bytes per element of this session's own KV cache (kc / vc): 2 bf16, 4 fp32 (precision 2)
    int weight_format = 0;  // 0: bf16; 1: W8A16 — decoder linears stored as e4m3 + per-row scales for the decode GEMV;
                            // 2: fp8 — 1 + the prefill GEMMs run e4m3 x e4m3 on the K=128 scaled MFMA (W8A8)
                            // 3: W4A16 — decoder linears stored as MXFP4 nibbles + E8M0 block scales for the decode GEMV
    Buf s_cols, s_patches, s_vx, s_vxn, s_vqkv, s_vq, s_vk, s_vv, s_vattn, s_vh, s_sel, s_mid, s_feats;
    Buf s_xn, s_qkv, s_q, s_attn, s_h, s_kc, s_vc, s_xl;
    Buf pp_src, pp_sq, pp_tmp, pp_out, pp_tab, pp_f32;
    int s_capB = 0, s_capS = 0;  // false: a session created by vc_model_create_shared (weights belong to the parent)
    // derived
    int P, Tv, Kpatch, Kpad, hd, vhd, npart;
    std::vector<void*> owned;  // every weight allocation
    // Checkpoints bf16 cannot hold (the reference's: an fp16 LLM, builder.py:25-40, and an fp32 CLIP hub checkpoint cast to fp16,
    // clip_encoder.py:22-27): every matrix whose fp32 source had a value != bf16(value) keeps a second bf16 plane lo = bf16(w - hi)
    // of the same layout.  lo_of maps a hi plane (row-major, or the decode steps' packed copy) to it.  Precision modes "strict" and
    // "split" contract against hi + lo (w to ~16 mantissa bits; exact for fp16 values); the bf16 fast path uses hi alone.
    // Written while loading / finalizing only; sessions read their root's map.
    std::map<const void*, bf16_t*> lo_of;
    std::set<std::pair<const void*, size_t>> inexact_regions;   // (matrix, offset) of every loaded tensor that needed a lo plane
    Buf cvt_tmp;               // fp16-operand build: fp32 image of a bfloat16 checkpoint tensor on its way to the planes kernel
    unsigned* inexact_flag = nullptr;   // device word for the loader's check
    std::map<std::string, bool> need;
    // weights
    float *vit_cls = nullptr, *vit_pos = nullptr, *vit_pre_w = nullptr, *vit_pre_b = nullptr;
    bf16_t* vit_patch_w = nullptr;
    std::vector<VitLayer> vit;
    std::vector<LlmLayer> llm;
    Projector mm, seg;
    bf16_t *embed = nullptr, *lm_head = nullptr, *lm_head_p = nullptr;
    float* final_norm = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    // staging
    Buf stage, stage2;
    // ViT workspace
    Buf v_pixels, v_cols, v_patches, v_x, v_xn, v_qkv, v_q, v_k, v_vt, v_attn, v_h, v_sel, v_mid, feats;
    int feat_rows[3] = {0, 0, 0}, feat_off[3] = {0, 0, 0};
    // list / 5-D image form (vcoder_ds_llava_arch.py:135-169): images per sample and modality for the NEXT prefill
    // (vc_set_image_counts; empty = one image per sample), and the running first-image index of every sample
    std::vector<int> img_counts[3], img_first[3];
    // padded batches: the caller's 2-D attention_mask for the NEXT prefill / generate (vc_set_attention_mask; one-shot), and
    // the left-extended key mask of the CURRENT prefill on the device ([VC_MAX_ROWS][max_positions] bytes, 1 = visible)
    std::vector<uint8_t> mask_next;
    int mask_B = 0, mask_T = 0;
    Buf kmask;
    bool has_kmask = false;         // the current prefill hides keys
    bool kmask_in_decode = false;   // ... and the session's decode steps keep hiding them (vc_decode_step loops)
    // output_hidden_states of the NEXT vc_prefill (vc_request_hidden_states; one-shot): host buffer [(L + 1), B, S, hidden]
    float* hidden_out = nullptr;
    size_t hidden_cap = 0;        // floats
    Buf hidden_tmp;
    // output_attentions of the NEXT vc_prefill (vc_request_attentions; one-shot): host buffer [L, B, H, S, S]
    float* attn_out = nullptr;
    size_t attn_cap = 0;
    Buf attn_q;                   // roped q of a decode step with output_attentions
    // token scores of the NEXT vc_prefill / vc_extend (vc_request_token_scores; one-shot): the caller's labels [B, T] (a copy), the host
    // buffers the call fills (cap elements each), and — while that call runs — score_on
    std::vector<int64_t> score_labels;
    int score_B = 0, score_T = 0;
    float* score_out = nullptr;
    int64_t* score_labels_out = nullptr;
    size_t score_cap = 0;
    bool score_on = false;
    std::vector<int64_t> spliced_labels;   // [B, S] of the prefill being scored (IGNORE_INDEX on feature rows and right padding)
    Buf sc_idx, sc_lp, sc_xn, sc_logits;   // scored rows: indices | targets, log-probs, normed rows and logits of one chunk
    // top-K alternatives of the scored positions (vc_request_top_logprobs; travels with the token-score request): the host buffers
    // [B, S] or [B, n] x top_k the scored call fills, cap entries each
    int stk_k = 0;
    float* stk_lp = nullptr;
    int32_t* stk_ids = nullptr;
    size_t stk_cap = 0;
    Buf sc_tlp, sc_tid;           // scored rows x top_k: log-probs and ids of one call
    // per-token log-probs of the NEXT vc_generate* (vc_request_generate_logprobs; one-shot): the host buffers [B, max_new] and
    // [B, max_new, top_k] (cap_rows rows each).  A call that runs on the session's loop attaches the slabs below (laid out like
    // out_ids: row stride out_stride) to its own copy of the loop's view: its steps then carry a topk_logprob launch behind their selection
    int glp_k = 0;
    float* glp_tok = nullptr;
    float* glp_top = nullptr;
    int32_t* glp_ids = nullptr;
    size_t glp_cap = 0;
    Buf lp_tok, lp_top, lp_ids;
    // logits processors of the NEXT vc_generate* (vc_request_logits_processors; one-shot), copied from the caller's struct: the
    // bad-word table as the kernel reads it ([VC_MAX_BAD_WORDS][1 + VC_MAX_BAD_WORD_LEN]: length, ids).  A call that runs on the
    // session's loop attaches proc_prompt / proc_bad (its prompt ids and table) and proc_logits (the processed rows [B, V]) to its own
    // copy of the loop's view: every selection is then preceded by logits_process_kernel
    bool gproc = false;
    float gproc_penalty = 1.f;
    int gproc_ngram = 0, gproc_minnew = 0, gproc_nbad = 0, gproc_neos = 0;
    int gproc_eos[VC_MAX_EOS_EXTRA] = {};
    std::vector<int> gproc_bad;
    Buf proc_prompt, proc_bad, proc_logits;
    // token automaton of the NEXT vc_generate (vc_request_constraint; one-shot), validated and copied from the caller's tables:
    // state_off [S + 1] | edge_tok [E] | edge_next [E] | default_next [S] in one vector, uploaded as it stands to cn_tab when a
    // call is armed.  Such a call runs on the session's loop with the processor launch in its steps (GenParams::cn), whose fourth
    // phase masks the processed rows
    std::vector<int> gcn_tab;
    int gcn_S = 0, gcn_E = 0;
    Buf cn_tab;
    // prompt-lookup speculation of the NEXT vc_generate* (vc_request_speculation; one-shot): k drafts per step, the largest n-gram,
    // the caller's lookup ids [B][spec_lookup_stride] with their lengths.  A call that serves it runs verify steps (STEP_SPEC) over
    // B * (k + 1) rows on the sp_* buffers; spec_counters [B][4] (steps, tokens, drafted, accepted) of the last call when spec_last.
    // spec_any (vc_request_speculation_selection; travels with the request): sampled calls and calls with processors are served too
    int spec_k = 0, spec_ngram = 0, spec_B = 0, spec_lookup_stride = 0;
    bool spec_any = false;
    std::vector<int> spec_lookup, spec_lookup_len;
    bool spec_last = false;
    bool spec_closed = false;     // a speculated call left the rows at different positions: the session's loop is closed
    std::vector<int> spec_counters;
    Buf sp_x, sp_xg, sp_qkv, sp_attn, sp_h, sp_logits, sp_ssq, sp_tok, sp_state, sp_lookup, sp_prompt, sp_lp, sp_ids;
    Buf sp_sel, sp_chosen, sp_proc;   // the wider scope: selections and their log-probs [B * Q], processed rows [B * Q, V]
    // fan-out of the NEXT vc_generate (vc_request_fanout; one-shot): n sequences per prompt.  A served call prefills the B prompts
    // once into rows 0 .. B - 1 of a cache of fan_rows = B n rows (fan_rows is set around that prefill only) and steps the B n rows with
    // the fan-out attention; fan_P holds the groups' prompt lengths.  fan_last*: what the last vc_generate made of a request
    int fan_n = 0, fan_rows = 0;
    bool fan_share = true;        // false: the caller asked for the repeated prompts (vc_request_fanout(-n))
    Buf fan_P;
    Buf fan_px[3];                // the pixels of a request that is not served, every sample's images n times
    bool fan_closed = false;      // a served fan-out call ran: cache row r no longer holds one sequence — the session's loop is closed
    bool fan_last = false, fan_last_shared = false;
    int fan_last_n = 0, fan_last_B = 0;
    // classifier-free guidance of the NEXT vc_generate / vc_prefill (vc_request_guidance; one-shot): the scale, a copy of the negative
    // prompt's ids [gd_B, gd_T] and the caller's pixel pointers of its images (borrowed until that call returns).  A served call runs
    // on the session's loop over 2 gd_B rows — the conditional rows 0 .. B - 1, their followers behind them — with the guided
    // selection tail (LoopView::gd_logits); gd_last*: what the last vc_generate / vc_prefill made of a request
    bool gd_on = false;
    float gd_scale = 1.f;
    std::vector<int64_t> gd_ids;
    int gd_B = 0, gd_T = 0, gd_px_on_dev = 0;
    const float* gd_px[3] = {nullptr, nullptr, nullptr};
    Buf gd_logits, gd_scalars;
    bool gd_closed = false;       // a guided generate ran: the rows stand at different positions — the session's loop is closed
    int gd_pair = 0;              // > 0: a guided vc_prefill left a loop of 2 gd_pair rows (pairs at different positions) for vc_decode_step
    bool gd_last = false;
    int gd_last_B = 0, gd_last_Sc = 0, gd_last_Sn = 0;
    // the further warpers of the NEXT vc_generate (vc_request_sampling_warpers; one-shot): min_p, typical_p, epsilon_cutoff,
    // eta_cutoff of a sampled call — 0 (typical_p: also >= 1) is off.  They travel in the rows' records (RS_MINP .. RS_ETA) and
    // change neither the loop a call runs on nor a captured step
    float warp_min_p = 0.f, warp_typical = 0.f, warp_eps = 0.f, warp_eta = 0.f;
    bool tok_stale = false;       // vc_rewind ran: the token the last step selected on the device no longer continues the sequence
    bool plan_only = false;       // do_prefill stops behind the splice plan (vc_plan_spliced_len): no tower pass, no state change
    int reserve_new = 64;         // KV slots a vc_prefill keeps free behind the prompt (vc_model_reserve_decode)
    int layer_limit = 0;          // > 0: a prefill evaluates only the first layer_limit decoder layers (vc_model_set_layer_limit)
    // LLM workspace
    Buf x, xn, qkv, q, attn, h, kc, vc, vt_pre, row_src, last_idx, xl, logits_all;
    Buf k_pre;                    // bf16 K rows of the current prefill layer when the cache holds e4m3 rows (fp8 format)
    Buf p_ssq, p_rstd;            // prefill: sum-of-squares partials [B*S, npart] and 1/rms [B*S] of the folded RMSNorm
    Buf a8, a8_scale;             // weight format 2: e4m3 activation rows of the current prefill GEMM + their scales
    int capB = 0, capS = 0;  // KV capacity
    int curB = 0, curS = 0, cur_pos = -1;
    // decode state of this session's own loop (vc_prefill / vc_decode_step, strict mode, generate with the pool off)
    Buf x_dec, xg_dec, qkv_dec, attn_dec, h_dec, logits, next_tok, out_ids, rows, dsum, ssq;
    Buf sk_scratch, sk_counters;  // split-K partials / arrival counters of the decode GEMV (few-tile matrices)
    Buf ext_tok;                  // token ids of a vc_extend call [B, n]
    Buf gemm_ws;                  // fp32 workspace of the GEMM's split-K remainder round (64 MiB)
    int out_stride = 0;           // out_ids ints per row
    int last_S = 0;               // spliced prompt length of the last prefill / generate
    // the captured decode steps of the session's loop, one per kind (StepKind above): each is replayed while the description
    // of the step a caller asks for equals the one it was captured from (StepKey: every address and size the launches bake in), and
    // re-captured otherwise.  The per-row parameters live in the RowState records, not in the graph.
    StepGraph step[STEP_KINDS];
    int step_captures = 0;        // captures of this session so far (vc_debug_step_captures)
    // the device beam loop (vc_generate_beam; BeamLoop): bm_state holds the fixed-size part (candidates, beam scores, perm, prompt
    // lengths, sequence records, hypotheses, parameters, flags), bm_tab the tok / parent tables, bm_den the two denominator tables,
    // bm_tmp the staging of the tail permute — the last three sized for bm_cap_new steps
    Buf bm_state, bm_tab, bm_den, bm_tmp;
    int bm_cap_new = 0;
    struct vc_pool* pool = nullptr;  // the root model's shared decode pool (created on first use; sessions point at it)
    bool pool_profile = false;       // root model: the pool's step graphs carry in-situ timing stamps (vc_pool_profile)
    bool fp8_kv = true;              // weight format 2: the KV cache of the bf16-step modes in e4m3 (vc_model_set_fp8_kv)
    bool batch_invariant = false;    // root model: a sample's bits do not depend on the batch it runs in (vc_model_set_batch_invariant)
    int qkv_fused = 1;               // root model: RoPE + head split + KV write in the prefill's QKV GEMM epilogue (vc_model_set_qkv_fused):
                                     // 0 off, 1 for problems the 256 x 256 GEMM kernel serves anyway (>= 1024 token rows), 2 always
    int pool_rows = VC_POOL_ROWS;    // root model: rows of the decode pool when it is next built (vc_pool_set_rows)
    std::atomic<bool> pool_hold{true};   // root model: the pool does not step while a call holding rows is still prefilling
                                         // (vc_pool_set_hold; written by any caller thread, read by the pool's driver thread)
    vc_model* root = nullptr;        // the model that owns the weights (itself for a root)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float t_encode = 0, t_prefill = 0, t_decode = 0;
};

struct vc_pool;
namespace {
void pool_destroy(vc_pool* p);
}

namespace {
#include "engine_weights.inc"
#include "engine_linears.inc"
#include "engine_vision.inc"
#include "engine_llm.inc"
}  // namespace

static void clear_score_request(vc_model* m) {
    m->score_labels.clear();
    m->score_B = m->score_T = 0;
    m->score_out = nullptr;
    m->score_labels_out = nullptr;
    m->score_cap = 0;
    m->score_on = false;
    m->stk_k = 0;
    m->stk_lp = nullptr;
    m->stk_ids = nullptr;
    m->stk_cap = 0;
}
static void clear_logits_processors_request(vc_model* m) {
    m->gproc = false;
    m->gproc_bad.clear();
}
static void clear_constraint_request(vc_model* m) {
    m->gcn_tab.clear();
    m->gcn_S = m->gcn_E = 0;
}
static void clear_speculation_request(vc_model* m) {
    m->spec_k = m->spec_ngram = m->spec_B = m->spec_lookup_stride = 0;
    m->spec_any = false;
    m->spec_lookup.clear();
    m->spec_lookup_len.clear();
}
static void clear_guidance_request(vc_model* m) {
    m->gd_on = false;
    m->gd_scale = 1.f;
    m->gd_ids.clear();
    m->gd_B = m->gd_T = m->gd_px_on_dev = 0;
    for (auto& p : m->gd_px) p = nullptr;
}
static void clear_sampling_warpers_request(vc_model* m) { m->warp_min_p = m->warp_typical = m->warp_eps = m->warp_eta = 0.f; }
static void clear_generate_logprobs_request(vc_model* m) {
    m->glp_k = 0;
    m->glp_tok = m->glp_top = nullptr;
    m->glp_ids = nullptr;
    m->glp_cap = 0;
}

// the one-shot requests of the NEXT prefill / generate call (vc_set_image_counts, vc_set_attention_mask,
// vc_request_hidden_states) never outlive that call — also not when it fails half-way (a stale mask would be applied to,
// and a stale host pointer written by, some later call)
struct OneShotReset {
    vc_model* m;
    ~OneShotReset() {
        for (auto& v : m->img_counts) v.clear();
        m->mask_next.clear();
        m->hidden_out = nullptr;
        m->hidden_cap = 0;
        m->attn_out = nullptr;
        m->attn_cap = 0;
        clear_score_request(m);
        clear_generate_logprobs_request(m);
        clear_logits_processors_request(m);
        clear_constraint_request(m);
        clear_speculation_request(m);
        clear_guidance_request(m);
        clear_sampling_warpers_request(m);
        m->fan_n = 0;
        m->fan_rows = 0;
    }
};

#include "engine_abi.inc"
#include "engine_pool.inc"
#include "engine_profile.inc"
