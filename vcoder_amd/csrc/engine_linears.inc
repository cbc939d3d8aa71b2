// engine_linears.inc — part of the host engine (textually included by engine.hip inside its anonymous namespace; one translation unit).
// GEMM / GEMV call helpers of the engine (split-K workspace, folded RMSNorm, the fused QKV epilogue's arguments), the GEMVs of one decode step.

// ------------------------------------------------------------------------------------------------
// GEMM helpers
// vc_model_set_batch_invariant: no split-K remainder round (its slices — and so the order in which a row's k-blocks are summed —
// depend on the number of output tiles, i.e. on how many rows share the launch)
inline bool batch_invariant(const vc_model* m) { return root_of(m)->batch_invariant; }
inline bool prefill_fold_on() {
    const char* e = getenv("VC_PREFILL_FOLD");
    return e && atoi(e) != 0;
}
// folded RMSNorm of a prefill (GemmArgs::row_scale / xg_out): what a GEMM consumes and what it hands to the next one
struct NormFold {
    const float* row_scale = nullptr;   // consumer: 1/rms per row
    bf16_t* xg_out = nullptr;           // producer (EPI_RESID_F32): the next GEMM's operand rows ...
    const float* xg_w = nullptr;        // ... = bf16(x * xg_w)
    float* ssq_out = nullptr;
    int ld_xg = 0, xg_lo = 0, npart = 0;
};
static void apply_fold(GemmArgs& a, const NormFold* f) {
    if (!f) return;
    a.row_scale = f->row_scale;
    a.xg_out = f->xg_out;
    a.xg_w = f->xg_w;
    a.ssq_out = f->ssq_out;
    a.ld_xg = f->ld_xg;
    a.xg_lo = f->xg_lo;
    a.npart = f->npart;
}
// the fp32 workspace of the GEMM's split-K remainder round: only problems with more than one round of tiles can use it
static void attach_splitk_ws(vc_model* m, GemmArgs& a) {
    if (batch_invariant(m) || (long)((a.M + 255) / 256) * ((a.N + 255) / 256) <= 256) return;
    m->gemm_ws.ensure((size_t)64 << 20);
    a.ws = m->gemm_ws.as<float>();
    a.ws_bytes = m->gemm_ws.cap;
}
void gemm(vc_model* m, const bf16_t* A, const bf16_t* W, const float* bias, void* out, int M, int N, int K, int ldo,
          int epi, int lda = 0, const NormFold* fold = nullptr, const QkvEpiArgs* qe = nullptr) {
    GemmArgs a{A, W, bias, out, M, N, K, lda > 0 ? lda : K, K, ldo};
    apply_fold(a, fold);
    if (qe) a.qe = *qe;
    attach_splitk_ws(m, a);
    launch_gemm(a, epi, m->st);
}
// weight format 2 (W8A8 prefill): the token rows of A are quantised to e4m3 with per-row power-of-two scales, then
// out = epi((Q @ Wq^T) * a_scale[m] * w_scale[n]) on the K=128 scaled MFMA
// A == nullptr: the e4m3 rows and scales are already in m->a8 / m->a8_scale (launch_rmsnorm_q8)
void gemm_f8(vc_model* m, const bf16_t* A, const uint8_t* Wq, const float* wscale, void* out, int M, int N, int K, int ldo,
             int epi, const QkvEpiArgs* qe = nullptr) {
    if (A) launch_quant_act_rows(A, K, m->a8.as<uint8_t>(), m->a8_scale.as<float>(), M, K, m->st);
    GemmArgs a{reinterpret_cast<const bf16_t*>(m->a8.p), reinterpret_cast<const bf16_t*>(Wq), nullptr, out, M, N, K, K, K, ldo};
    if (qe) a.qe = *qe;
    attach_splitk_ws(m, a);
    a.f8 = 1;
    a.a_scale = m->a8_scale.as<float>();
    a.w_scale = wscale;
    launch_gemm(a, epi, m->st);
}
// precision mode "split": A is the K-concatenated [hi | lo] bf16 image of an fp32 activation matrix (row stride lda >= 2 Kw),
// W [N, Kw] is contracted against both halves (kwrap); split_out > 0: a bf16-valued epilogue writes [hi | lo] again, the lo
// plane split_out columns to the right
void gemm_split(vc_model* m, const bf16_t* A, const bf16_t* W, const float* bias, void* out, int M, int N, int Kw, int ldo,
                int epi, int lda, int split_out = 0, const NormFold* fold = nullptr) {
    GemmArgs a{A, W, bias, out, M, N, 2 * Kw, lda, Kw, ldo};
    a.kwrap = Kw / 64;
    a.split_out = split_out;
    if (const bf16_t* Wl = lo_plane(m, W)) {   // an inexact checkpoint: a third K segment, a_hi . w_lo (gemm.hip w_koff)
        a.K = 3 * Kw;
        a.w_lo_off = (long long)(reinterpret_cast<const char*>(Wl) - reinterpret_cast<const char*>(W));
    }
    apply_fold(a, fold);
    attach_splitk_ws(m, a);
    launch_gemm(a, epi, m->st);
}
// row stride of a [hi | lo] operand of width K: padded like XN_PAD (2 K bf16 is a power-of-two stride at K = 4096)
inline int split_ld(int K) { return 2 * K + XN_PAD; }

// split-K buffers of the decode GEMVs: the widest [K-slices][output tiles] product of the model's matrices (the workgroup-shared
// form slices qkv / gate-up / lm_head as well: at most 8 slices, decode.hip wg_geometry), two row groups of 256 floats each
inline size_t sk_floats(const vc_model_cfg& c) {
    const size_t tiles = (size_t)std::max(std::max(3 * c.hidden, 2 * c.ffn), c.vocab) / 16 + 1;
    return std::max((size_t)4 * 512, (size_t)8 * tiles) * 2 * 256;
}
inline int sk_counters_n(const vc_model_cfg& c) { return (int)((size_t)std::max(std::max(3 * c.hidden, 2 * c.ffn), c.vocab) / 16 + 1) * 2; }

// bytes per KV-cache element of precision mode "split": 3 = fp24 (default: hd x u16 | hd x u8 per row, 2^-17 relative, 0.75 of the
// fp32 bytes the decode attention streams), 4 = fp32 (VC_SPLIT_KV=32: regression / A-B)
inline int split_kv_es() {
    static const int es = (getenv("VC_SPLIT_KV") && atoi(getenv("VC_SPLIT_KV")) == 32) ? 4 : 3;
    return es;
}

// the fp8 weight format (2) keeps its KV cache in e4m3 as well (1 byte per element: at 13b the pooled decode attention reads 2.6x
// the bytes of the e4m3 weights otherwise); vc_model_set_fp8_kv(m, 0) keeps bf16 rows (root model's setting, before finalize)
// bytes per KV element of the bf16-step modes (precision 0) of a model
inline int step_kv_es(const vc_model* m) {
    const vc_model* r = root_of(m);
    return (r->weight_format == 2 && r->fp8_kv) ? 1 : 2;
}

// the next timing slot of the step being enqueued (nullptr: profiling off)
inline unsigned* next_stamp(const LoopView& v) {
    if (!v.stamps || !v.stamp_next) return nullptr;
    return v.stamps + STAMP_SLOT_WORDS * (size_t)(*v.stamp_next)++;
}

// decode-time linear over `X` (bf16 [M, K]).  use_rstd: X is the xg operand (bf16(x * g)) and the output is scaled by the
// rows' 1/rms from the ssq partials; next_norm_w (RESID epilogue only): publish the ssq partials of the updated residual
// rows and the next consumer's xg operand
// split decode step (v.split_G = G): X and every bf16-valued output are stacked groups of G hi rows + G lo rows, one
// weight pass serves one group (G rows: hi + lo fill the kernel's 16 / 32 token slots)
void gemv(vc_model* m, const LoopView& v, const bf16_t* X, const bf16_t* Wp, const float* wscale, void* out, int M, int N, int K,
          int ldo, int epi, bool use_rstd = false, const float* next_norm_w = nullptr) {
    const bool f32out = epi == GEMV_F32 || epi == GEMV_RESID_F32;
    const size_t esz = f32out ? 4 : 2;
    const int np = m->npart;
    const int G = v.split_G;
    const int pass = G ? G : VC_GEMV_MAX_M;
    for (int m0 = 0; m0 < M; m0 += pass) {  // the skinny kernel holds VC_GEMV_MAX_M token slots per weight pass
        const size_t xrow0 = G ? (size_t)(m0 / G) * 2 * G : (size_t)m0;   // first row of the pass in a stacked bf16 buffer
        GemvArgs a{};
        a.X = X + xrow0 * K;
        a.Wp = Wp;
        // W4A16 keeps its E8M0 block-scale bytes where the e4m3 formats keep their per-row scales (lm_head: bf16, no scales)
        if (root_of(m)->weight_format == 3 && wscale != nullptr) a.w4scale = reinterpret_cast<const uint8_t*>(wscale);
        else a.wscale = wscale;
        a.out = reinterpret_cast<char*>(out) + (f32out ? (size_t)m0 : xrow0) * ldo * esz;
        a.M = std::min(pass, M - m0);
        a.N = N;
        a.K = K;
        a.ldo = ldo;
        a.split_rows = G;
        a.ssq_in = use_rstd ? v.ssq + (size_t)m0 * np : nullptr;
        if (next_norm_w) {
            a.ssq_out = v.ssq + (size_t)m0 * np;
            a.xg_w = next_norm_w;
            a.xg_out = v.xg_dec + xrow0 * N;
        }
        a.npart = np;
        a.eps = m->c.rms_eps;
        // the launcher may split K over several workgroups per tile (per-wave rings: o_proj / down only; the workgroup-shared
        // form: any matrix)
        a.sk_scratch = v.sk_scratch;
        a.sk_counters = v.sk_counters;
        a.sk_scratch_floats = sk_floats(m->c);
        a.sk_counters_n = sk_counters_n(m->c);
        a.stamp = next_stamp(v);
        if (G) a.Wp_lo = lo_plane(m, Wp);   // split mode on an inexact checkpoint
        launch_gemv(a, epi, v.st);
    }
}

// the GEMVs of one decode step over the first M rows; `between(l)` runs after the qkv projection of layer l (the attention)
template <class F, class G>
void decode_linears(vc_model* m, const LoopView& v, int M, F&& between, G&& after_layer) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, Fd = c.ffn;
    const bf16_t* xg = v.xg_dec;
    for (int l = 0; l < c.layers; ++l) {
        const LlmLayer& L = m->llm[l];
        const float* next_in = l + 1 < c.layers ? m->llm[l + 1].in_norm : m->final_norm;
        gemv(m, v, xg, L.qkv_p, L.qkv_s, v.qkv_dec, M, 3 * D, D, 3 * D, v.split_G ? GEMV_F32 : GEMV_BF16, true);  // K11+K12
        between(l);                                                                                          // K13-K15
        gemv(m, v, v.attn_dec, L.o_p, L.o_s, v.x_dec, M, D, D, D, GEMV_RESID_F32, false, L.post_norm);          // K16
        gemv(m, v, xg, L.gu_p, L.gu_s, v.h_dec, M, 2 * Fd, D, Fd, GEMV_SWIGLU, true);                          // K11+K17
        gemv(m, v, v.h_dec, L.down_p, L.down_s, v.x_dec, M, D, Fd, D, GEMV_RESID_F32, false, next_in);          // K17
        after_layer(l);
    }
    gemv(m, v, xg, m->lm_head_p, nullptr, v.logits, M, c.vocab, D, c.vocab, GEMV_F32, true);                    // K11+K18
}
template <class F>
void decode_linears(vc_model* m, const LoopView& v, int M, F&& between) {
    decode_linears(m, v, M, between, [](int) {});
}

