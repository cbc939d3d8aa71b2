// engine_abi.inc — part of the host engine (textually included by engine.hip): the model-level C entry points of include/vcoder_hip.h —
// init, model create / load / finalize, the mode setters, encode, prefill, decode_step, cache reorder.

// =================================================================================================
// C ABI
// =================================================================================================
#define GUARD_BEGIN try {
// the HIP current device is per host thread: sessions may be driven from any thread
#define USE_DEVICE(ctxp)                       \
    do {                                       \
        HIPCHK(hipSetDevice((ctxp)->device)); \
        t_stream = (ctxp)->stream;             \
    } while (0)
// The HIP runtime keeps a per-thread "last error" that a LATER caller of hipGetLastError() — torch checks it after its own
// launches — would inherit from a query of ours that legitimately returned non-success (hipEventQuery: not ready, ...).
// Every entry point leaves it clean; VC_DEBUG_HIP=1 reports what it found.
#define CLEAR_HIP_LAST_ERROR(where)                                                                  \
    do {                                                                                             \
        hipError_t le_ = hipGetLastError();                                                          \
        if (le_ != hipSuccess && getenv("VC_DEBUG_HIP"))                                             \
            fprintf(stderr, "[vcoder_amd] %s left HIP last-error %d (%s)\n", where, (int)le_, hipGetErrorString(le_)); \
    } while (0)
#define GUARD_END(ctxp)                                   \
    }                                                     \
    catch (const Fail& f) {                               \
        if (ctxp) (ctxp)->err = f.msg;                    \
        CLEAR_HIP_LAST_ERROR(__func__);                   \
        return f.code;                                    \
    }                                                     \
    catch (const std::exception& e) {                     \
        if (ctxp) (ctxp)->err = e.what();                 \
        CLEAR_HIP_LAST_ERROR(__func__);                   \
        return VC_ERR_INVALID;                            \
    }                                                     \
    CLEAR_HIP_LAST_ERROR(__func__);                       \
    return VC_OK;

VC_API int vc_init(int device_id, vc_ctx** out) {
    if (!out) return VC_ERR_INVALID;
    *out = nullptr;
    vc_ctx* ctx = new vc_ctx();
    GUARD_BEGIN
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    REQUIRE(n > 0 && device_id >= 0 && device_id < n, VC_ERR_HIP, "no HIP device %d (found %d)", device_id, n);
    HIPCHK(hipSetDevice(device_id));
    ctx->device = device_id;
    ctx->stream = make_stream();
    *out = ctx;
    GUARD_END(ctx)
}
VC_API void vc_shutdown(vc_ctx* ctx) {
    if (!ctx) return;
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}
VC_API const char* vc_last_error(vc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
VC_API int vc_synchronize(vc_ctx* ctx) {
    GUARD_BEGIN
    USE_DEVICE(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    GUARD_END(ctx)
}
VC_API void* vc_stream(vc_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

VC_API int vc_model_create(vc_ctx* ctx, const vc_model_cfg* cfg, vc_model** out) {
    if (!ctx || !cfg || !out) return VC_ERR_INVALID;
    *out = nullptr;
    vc_model* m = nullptr;
    GUARD_BEGIN
    USE_DEVICE(ctx);
    const vc_model_cfg& c = *cfg;
    REQUIRE(c.variant >= 0 && c.variant <= 2, VC_ERR_INVALID, "bad variant %d", c.variant);
    REQUIRE(c.hidden % c.heads == 0 && c.vit_hidden % c.vit_heads == 0, VC_ERR_INVALID, "hidden %% heads != 0");
    const int hd = c.hidden / c.heads, vhd = c.vit_hidden / c.vit_heads;
    REQUIRE((hd == 128 || hd == 64) && (vhd == 64 || vhd == 128), VC_ERR_INVALID,
            "head dims (%d LLM, %d ViT) must be 64 or 128", hd, vhd);
    REQUIRE(c.hidden % 64 == 0 && c.ffn % 64 == 0 && c.vit_hidden % 64 == 0 && c.vit_ffn % 64 == 0 && c.vocab % 16 == 0,
            VC_ERR_INVALID, "hidden/ffn sizes must be multiples of 64 and vocab of 16");
    REQUIRE(c.vit_layers_used >= 0 && c.vit_layers_used <= c.vit_layers, VC_ERR_INVALID, "bad vit_layers_used");
    REQUIRE(c.vit_image % c.vit_patch == 0, VC_ERR_INVALID, "image size must be a multiple of the patch size");
    REQUIRE(c.mm_proj_depth >= 0 && c.seg_proj_depth >= 0, VC_ERR_INVALID, "bad projector depth");
    REQUIRE(c.max_positions >= 64 && c.max_positions <= 4096, VC_ERR_INVALID,
            "max_positions %d: the decode attention keeps a row's scores in LDS (<= 4096 keys)", c.max_positions);
    m = new vc_model();
    m->ctx = ctx;
    m->c = c;
    m->st = ctx->stream;
    m->hd = hd;
    m->vhd = vhd;
    const int g = c.vit_image / c.vit_patch;
    m->P = g * g;
    m->Tv = m->P + 1;
    m->Kpatch = 3 * c.vit_patch * c.vit_patch;
    m->Kpad = (int)rup(m->Kpatch, 64);
    m->npart = (int)rup(c.hidden / 16, 16);
    const int D = c.hidden, F = c.ffn, V = c.vocab, Dv = c.vit_hidden, Fv = c.vit_ffn;
    m->embed = walloc<bf16_t>(m, (size_t)V * D);
    m->lm_head = walloc<bf16_t>(m, (size_t)V * D);
    m->final_norm = walloc<float>(m, D);
    m->llm.resize(c.layers);
    for (auto& L : m->llm) {
        L.in_norm = walloc<float>(m, D);
        L.post_norm = walloc<float>(m, D);
        L.qkv_w = walloc<bf16_t>(m, (size_t)3 * D * D);
        L.o_w = walloc<bf16_t>(m, (size_t)D * D);
        L.gate_tmp = walloc<bf16_t>(m, (size_t)F * D);
        L.up_tmp = walloc<bf16_t>(m, (size_t)F * D);
        L.gu_w = walloc<bf16_t>(m, (size_t)2 * F * D);
        L.down_w = walloc<bf16_t>(m, (size_t)D * F);
        L.qkv_p = L.o_p = L.gu_p = L.down_p = nullptr;
    }
    auto mkproj = [&](Projector& pj, int depth) {
        pj.depth = depth;
        for (int l = 0; l < depth; ++l) {
            pj.w.push_back(walloc<bf16_t>(m, (size_t)D * (l == 0 ? Dv : D)));
            pj.b.push_back(walloc<float>(m, D));
        }
    };
    mkproj(m->mm, c.mm_proj_depth);
    if (c.variant != VC_VARIANT_LLAVA) mkproj(m->seg, c.seg_proj_depth);
    m->vit_cls = walloc<float>(m, Dv);
    m->vit_pos = walloc<float>(m, (size_t)m->Tv * Dv);
    m->vit_pre_w = walloc<float>(m, Dv);
    m->vit_pre_b = walloc<float>(m, Dv);
    m->vit_patch_w = walloc<bf16_t>(m, (size_t)Dv * m->Kpad, true);
    m->vit.resize(c.vit_layers_used);
    for (auto& L : m->vit) {
        L.ln1_w = walloc<float>(m, Dv); L.ln1_b = walloc<float>(m, Dv);
        L.ln2_w = walloc<float>(m, Dv); L.ln2_b = walloc<float>(m, Dv);
        L.qkv_w = walloc<bf16_t>(m, (size_t)3 * Dv * Dv); L.qkv_b = walloc<float>(m, 3 * Dv);
        L.out_w = walloc<bf16_t>(m, (size_t)Dv * Dv); L.out_b = walloc<float>(m, Dv);
        L.fc1_w = walloc<bf16_t>(m, (size_t)Fv * Dv); L.fc1_b = walloc<float>(m, Fv);
        L.fc2_w = walloc<bf16_t>(m, (size_t)Dv * Fv); L.fc2_b = walloc<float>(m, Dv);
    }
    mark_needed(m);
    for (auto& e : m->ev) HIPCHK(hipEventCreate(&e));
    *out = m;
    GUARD_END(ctx)
}

/* A second SESSION on the same weights: own stream (the new ctx), own workspaces / KV cache / hipGraph; weight tensors are
 * shared read-only with `parent` (which must be finalized and must outlive the session).  Several sessions let the GPU
 * overlap one batch's MFMA-bound prefill and per-launch ramps with another batch's HBM-bound decode. */
VC_API int vc_model_create_shared(vc_ctx* ctx, vc_model* parent, vc_model** out) {
    if (!ctx || !parent || !out) return VC_ERR_INVALID;
    *out = nullptr;
    GUARD_BEGIN
    USE_DEVICE(ctx);
    REQUIRE(parent->finalized, VC_ERR_STATE, "parent model is not finalized");
    vc_model* m = new vc_model();
    m->ctx = ctx;
    m->c = parent->c;
    m->st = ctx->stream;
    m->finalized = true;
    m->owns_weights = false;
    m->root = root_of(parent);
    m->weight_format = parent->weight_format;
    m->P = parent->P; m->Tv = parent->Tv; m->Kpatch = parent->Kpatch; m->Kpad = parent->Kpad;
    m->hd = parent->hd; m->vhd = parent->vhd; m->npart = parent->npart;
    m->vit_cls = parent->vit_cls; m->vit_pos = parent->vit_pos; m->vit_pre_w = parent->vit_pre_w;
    m->vit_pre_b = parent->vit_pre_b; m->vit_patch_w = parent->vit_patch_w;
    m->vit = parent->vit; m->llm = parent->llm; m->mm = parent->mm; m->seg = parent->seg;
    m->embed = parent->embed; m->lm_head = parent->lm_head; m->lm_head_p = parent->lm_head_p;
    m->final_norm = parent->final_norm; m->rope_cos = parent->rope_cos; m->rope_sin = parent->rope_sin;
    for (auto& e : m->ev) HIPCHK(hipEventCreate(&e));
    *out = m;
    GUARD_END(ctx)
}

VC_API void vc_model_destroy(vc_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->st);
    if (m->pool) {  // the root's decode pool (sessions must be gone: they prefill into its rows)
        pool_destroy(m->pool);
        m->pool = nullptr;
    }
    drop_graph(m);   // (StepKey: the model's life is no key member)
    if (m->owns_weights)
        for (void* p : m->owned) (void)hipFree(p);
    for (Buf* b : {&m->stage, &m->stage2, &m->v_pixels, &m->v_cols, &m->v_patches, &m->v_x, &m->v_xn, &m->v_qkv, &m->v_q,
                   &m->v_k, &m->v_vt, &m->v_attn, &m->v_h, &m->v_sel, &m->v_mid, &m->feats, &m->x, &m->xn, &m->qkv, &m->q,
                   &m->attn, &m->h, &m->kc, &m->vc, &m->vt_pre, &m->row_src, &m->last_idx, &m->xl, &m->logits_all, &m->x_dec,
                   &m->xg_dec, &m->qkv_dec, &m->attn_dec, &m->h_dec, &m->logits, &m->next_tok, &m->rows,
                   &m->out_ids, &m->dsum, &m->ssq, &m->sk_scratch, &m->sk_counters, &m->gemm_ws, &m->s_cols, &m->s_patches, &m->s_vx, &m->s_vxn, &m->s_vqkv,
                   &m->s_vq, &m->s_vk, &m->s_vv, &m->s_vattn, &m->s_vh, &m->s_sel, &m->s_mid, &m->s_feats, &m->s_xn, &m->s_qkv,
                   &m->s_q, &m->s_attn, &m->s_h, &m->s_kc, &m->s_vc, &m->s_xl, &m->pp_src, &m->pp_sq, &m->pp_tmp, &m->pp_out,
                   &m->pp_tab, &m->pp_f32, &m->kmask, &m->hidden_tmp, &m->attn_q, &m->a8, &m->a8_scale, &m->p_ssq, &m->p_rstd, &m->k_pre,
                   &m->ext_tok, &m->sc_idx, &m->sc_lp, &m->sc_xn, &m->sc_logits, &m->sc_tlp, &m->sc_tid, &m->lp_tok, &m->lp_top,
                   &m->lp_ids, &m->proc_prompt, &m->proc_bad, &m->proc_logits, &m->cn_tab, &m->bm_state, &m->bm_tab, &m->bm_den, &m->bm_tmp, &m->fan_P,
                   &m->fan_px[0], &m->fan_px[1], &m->fan_px[2], &m->sp_x, &m->sp_xg, &m->sp_qkv, &m->sp_attn, &m->sp_h, &m->sp_logits, &m->sp_ssq,
                   &m->sp_tok, &m->sp_state, &m->sp_lookup, &m->sp_prompt, &m->sp_lp, &m->sp_ids, &m->sp_sel, &m->sp_chosen, &m->sp_proc})
        b->release();
    for (auto& e : m->ev)
        if (e) (void)hipEventDestroy(e);
    delete m;
    CLEAR_HIP_LAST_ERROR("vc_model_destroy");
}

VC_API int vc_model_load_tensor(vc_model* m, const char* hf_key, const void* host_ptr, int dtype, const int64_t* shape,
                                int ndim) {
    if (!m) return VC_ERR_INVALID;
    int rc = VC_OK;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(hf_key && host_ptr && shape && ndim >= 1 && ndim <= 8, VC_ERR_INVALID, "bad load_tensor arguments");
    REQUIRE(dtype == VC_F32 || dtype == VC_BF16, VC_ERR_INVALID, "dtype must be VC_F32 or VC_BF16");
    REQUIRE(!m->finalized, VC_ERR_STATE, "model already finalized");
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    const size_t bytes = numel * (dtype == VC_F32 ? 4 : 2);
    m->stage.ensure(bytes);
    HIPCHK(hipMemcpyAsync(m->stage.p, host_ptr, bytes, hipMemcpyHostToDevice, m->st));
    rc = place_tensor(m, hf_key, m->stage.p, dtype, shape, ndim);
    HIPCHK(hipStreamSynchronize(m->st));
    if (rc != VC_OK) return rc;
    GUARD_END(m->ctx)
}

VC_API int vc_model_synth_tensor(vc_model* m, const char* hf_key, const int64_t* shape, int ndim, uint32_t tensor_seed,
                                 float offset, float halfwidth) {
    if (!m) return VC_ERR_INVALID;
    int rc = VC_OK;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(hf_key && shape && ndim >= 1 && ndim <= 8, VC_ERR_INVALID, "bad synth_tensor arguments");
    REQUIRE(!m->finalized, VC_ERR_STATE, "model already finalized");
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    REQUIRE(numel < ((size_t)1 << 32), VC_ERR_INVALID, "tensor too large for the 32-bit generator");
#if VC_OPERAND_FP16
    // the fp16-operand build: the generator's values (on the bfloat16 grid, as in every build) are staged as fp32 and take the fp32
    // load path — VC_BF16 sources are bfloat16 BITS, which is not what launch_synth_bf16 writes here
    m->stage.ensure(numel * 4);
    launch_synth_f32(m->stage.as<float>(), numel, tensor_seed, offset, halfwidth, m->st);
    rc = place_tensor(m, hf_key, m->stage.p, VC_F32, shape, ndim);
#else
    m->stage.ensure(numel * 2);
    launch_synth_bf16(m->stage.as<bf16_t>(), numel, tensor_seed, offset, halfwidth, m->st);
    rc = place_tensor(m, hf_key, m->stage.p, VC_BF16, shape, ndim);
#endif
    HIPCHK(hipStreamSynchronize(m->st));
    if (rc != VC_OK) return rc;
    GUARD_END(m->ctx)
}

/* The same generator with the value classes of the reference's own checkpoints: rounding 0 = bf16 (vc_model_synth_tensor), 1 = the
 * value an fp16 checkpoint holds, 2 = unrounded fp32 (vcoder_amd/synth.py synth_tensor(rounding=...)).  1 and 2 go through the fp32
 * load path, i.e. keep weight lo planes (vc_model_inexact_tensors). */
VC_API int vc_model_synth_tensor_rounded(vc_model* m, const char* hf_key, const int64_t* shape, int ndim, uint32_t tensor_seed,
                                         float offset, float halfwidth, int rounding) {
    if (!m) return VC_ERR_INVALID;
    if (rounding == 0) return vc_model_synth_tensor(m, hf_key, shape, ndim, tensor_seed, offset, halfwidth);
    int rc = VC_OK;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(hf_key && shape && ndim >= 1 && ndim <= 8 && (rounding == 1 || rounding == 2), VC_ERR_INVALID, "bad synth_tensor arguments");
    REQUIRE(!m->finalized, VC_ERR_STATE, "model already finalized");
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    REQUIRE(numel < ((size_t)1 << 32), VC_ERR_INVALID, "tensor too large for the 32-bit generator");
    m->stage.ensure(numel * 4);
    launch_synth_f32_rounded(m->stage.as<float>(), numel, tensor_seed, offset, halfwidth, rounding, m->st);
    rc = place_tensor(m, hf_key, m->stage.p, VC_F32, shape, ndim);
    HIPCHK(hipStreamSynchronize(m->st));
    if (rc != VC_OK) return rc;
    GUARD_END(m->ctx)
}

/* 0: bf16 MFMA path (default, benchmarked); 1: strict fp32 path (fp32 activations + fp32 MFMA, ~1e-6 from the fp32 CPU
 * reference; slow).  Takes effect at the next prefill. */
VC_API int vc_model_set_precision(vc_model* m, int mode) {
    if (!m || mode < 0 || mode > 2) return VC_ERR_INVALID;
    if (mode == 2) {
        // split mode on a checkpoint with weight lo planes: its decode GEMV is the workgroup-shared form only — refuse HERE what
        // would otherwise surface as an exception out of a launch (possibly inside a graph capture) (ADVICE r5)
        const vc_model* root = root_of(m);
        // (the e4m3 weight formats re-round the decoder linears and drop their lo planes: only K = hidden matrices keep one then)
        if (!root->lo_of.empty() && (!gemv_wg_enabled() || root->c.hidden % 64 != 0 || (root->weight_format == 0 && root->c.ffn % 64 != 0))) {
            m->ctx->err = std::string("precision mode split on a checkpoint with weight lo planes (fp16 / fp32 values) needs the workgroup-shared "
                              "decode GEMV (vck_set_gemv_variant != 0, hidden_size and intermediate_size multiples of 64)");
            return VC_ERR_STATE;
        }
    }
    if (mode != m->precision) {  // the captured steps bake m->precision in without it being a member of their key (StepKey)
        (void)hipSetDevice(m->ctx->device);
        (void)hipStreamSynchronize(m->st);
        drop_graph(m);
    }
    m->precision = mode;
    m->cur_pos = -1;
    return VC_OK;
}

/* 0: bf16 weights (default).  1: W8A16 — q/k/v/o/gate/up/down of every decoder layer are quantised at finalize to OCP
 * e4m3 with a per-output-row power-of-two scale; embeddings, lm_head, norms, the CLIP tower and the adapters stay
 * bf16/fp32.  2: fp8 (BASELINE config C5, "CDNA4 fp8 MFMA") — the same weights; the cached decode steps stream the bytes
 * as in 1 (bf16 activations), and the prefill's decoder linears additionally quantise their activation rows to e4m3
 * (per-token power-of-two scale) and run e4m3 x e4m3 on v_mfma_scale_f32_16x16x128_f8f6f4 at twice the bf16 MFMA rate.
 * 3: W4A16 — the same seven matrices as MXFP4 (OCP e2m1 elements, one power-of-two E8M0 scale per 32 consecutive k of a row); the
 * cached decode steps stream the nibbles (bf16 activations), everything else computes with the effective weights q * 2^e, which the
 * quantiser writes back over the row-major matrices.  Needs hidden and ffn sizes divisible by 128.
 * Must be called before vc_model_finalize. */
VC_API int vc_model_set_weight_format(vc_model* m, int fmt) {
    if (!m || fmt < 0 || fmt > 3) return VC_ERR_INVALID;
    if (m->finalized) return VC_ERR_STATE;
    m->weight_format = fmt;
    return VC_OK;
}

/* Weight format 2 ("fp8") keeps the KV cache of its decode steps in e4m3 as well (1 byte per element, unscaled, saturating at 448;
 * default on).  on = 0: bf16 rows, as the other formats.  Before vc_model_finalize. */
VC_API int vc_model_set_fp8_kv(vc_model* m, int on) {
    if (!m) return VC_ERR_INVALID;
    if (m->finalized) return VC_ERR_STATE;
    m->fp8_kv = on != 0;
    return VC_OK;
}

/* Batch invariance (SURVEY.md §0 quirk 6: the reference's rows do not depend on the batch size; §4 test 4: the gathered stream of
 * N ranks == the single-GPU stream of the same global batch).  By default a prefill GEMM whose last round of output tiles is short
 * cuts that round into K-slices, and the number of slices follows from the tile count — so a sample's low-order bits can differ
 * between a batch of 4 and two batches of 2 (1e-6-level; visible only through near-tied greedy choices).  on = 1: no remainder
 * split — every output row is summed in one fixed k order whatever shares its launch (the decode steps, attention and row kernels
 * already are), at the price of a short last round of tiles per GEMM (~2-4 % of a prefill).  Applies to all sessions of the model. */
VC_API int vc_model_set_batch_invariant(vc_model* m, int on) {
    if (!m) return VC_ERR_INVALID;
    root_of(m)->batch_invariant = on != 0;
    return VC_OK;
}

/* The prefill's QKV projection with RoPE + head split + KV-cache write in the GEMM's epilogue (default on; SURVEY K13): on = 0 runs the
 * two launches it replaces (EPI_BF16 GEMM + qkv_split_kernel) — same bits when the padded and the plain token count give the GEMM the
 * same tile rounds, A/B and regression switch; on = 2 takes the fused form for every problem size (default 1: from 1024 token rows,
 * where the 256 x 256 kernel is used anyway).  Applies to all sessions of the model. */
VC_API int vc_model_set_qkv_fused(vc_model* m, int on) {
    if (!m) return VC_ERR_INVALID;
    if (on < 0 || on > 2) return VC_ERR_INVALID;
    root_of(m)->qkv_fused = on;
    return VC_OK;
}

/* Parity diagnostic: the next prefills evaluate only the first n decoder layers (0 = all) and apply the final norm +
 * lm_head to that hidden state — the logits of the same checkpoint cut to n layers.  Lets a test chart how the bf16
 * path's deviation from the fp32 oracle grows with depth on ONE loaded model.  Decode steps always use every layer. */
VC_API int vc_model_set_layer_limit(vc_model* m, int n_layers) {
    if (!m || n_layers < 0) return VC_ERR_INVALID;
    m->layer_limit = n_layers;
    m->cur_pos = -1;
    return VC_OK;
}

/* 16-bit operand format this library was built for: 0 = bfloat16 (libvcoder_hip.so, the benchmarked path), 1 = IEEE fp16
 * (libvcoder_hip_f16.so: the same kernels built with -DVC_F16 — v_mfma_f32_16x16x32_f16, saturating fp16 conversions; the
 * precision of the reference's own GPU path, vcoder_llava/model/builder.py:39,142) */
VC_API int vc_operand_format(void) { return VC_OPERAND_FP16; }

/* Number of loaded tensors whose fp32 source held values bf16 cannot represent (an fp16 / fp32 checkpoint; 0 for a bf16 one).
 * Each keeps a bf16 lo plane: precision modes "strict" and "split" compute with hi + lo (the checkpoint's values to ~16 mantissa
 * bits, exact for fp16), the bf16 fast path with the bf16-rounded weights alone. */
VC_API int vc_model_inexact_tensors(vc_model* m) {
    if (!m) return VC_ERR_INVALID;
    const vc_model* r = root_of(m);
    return (int)r->inexact_regions.size();
}

VC_API int vc_model_finalize(vc_model* m) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    if (m->finalized) return VC_OK;
    for (auto& kv : m->need) REQUIRE(kv.second, VC_ERR_STATE, "missing tensor '%s'", kv.first.c_str());
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn, V = c.vocab;
    // decode copy of one decoder linear: MFMA-packed bf16, or (W8A16) e4m3 super-tiles + per-row scales — the quantiser
    // also rewrites the row-major bf16 matrix with the dequantised values so prefill and decode share one set of weights
    auto decode_copy = [&](bf16_t* W, int N, int K, bf16_t*& Wp, float*& Ws, uint8_t*& Wq) {
        if (m->weight_format == 3) {   // W4A16: nibbles + E8M0 block scale bytes (held in the layer's scale slot: engine_linears.inc gemv)
            Wp = reinterpret_cast<bf16_t*>(walloc<uint8_t>(m, (size_t)N * K / 2));
            Ws = reinterpret_cast<float*>(walloc<uint8_t>(m, (size_t)N * K / 32));
            Wq = nullptr;
            launch_quantize_mxfp4(W, reinterpret_cast<uint8_t*>(Wp), reinterpret_cast<uint8_t*>(Ws), N, K, m->st);
        } else if (m->weight_format >= 1) {
            Wp = reinterpret_cast<bf16_t*>(walloc<uint8_t>(m, (size_t)N * K));
            Ws = walloc<float>(m, N);
            Wq = m->weight_format == 2 ? walloc<uint8_t>(m, (size_t)N * K) : nullptr;
            launch_quantize_fp8(W, reinterpret_cast<uint8_t*>(Wp), Ws, N, K, m->st, Wq);
        } else {
            Wp = walloc<bf16_t>(m, (size_t)N * K);
            launch_pack_weight(W, Wp, N, K, m->st);
        }
    };
    if (m->weight_format == 3)
        REQUIRE(D % 128 == 0 && F % 128 == 0, VC_ERR_INVALID, "W4A16 (MXFP4) needs hidden and ffn sizes divisible by 128 (got %d, %d)", D, F);
    else if (m->weight_format >= 1)
        REQUIRE(D % 64 == 0 && F % 64 == 0, VC_ERR_INVALID, "W8A16 needs hidden and ffn sizes divisible by 64");
    if (m->weight_format == 2)
        REQUIRE(D % 128 == 0 && F % 128 == 0, VC_ERR_INVALID, "the fp8 prefill GEMM needs hidden and ffn sizes divisible by 128");
    // lo planes of an inexact checkpoint (m->lo_of): interleaved / packed like their hi planes; the e4m3 weight formats re-round
    // the decoder linears anyway, so those drop theirs
    auto free_owned = [&](void* p) {
        for (auto& o : m->owned)
            if (o == p) { (void)hipFree(o); o = nullptr; }
    };
    auto drop_lo = [&](const void* hi) {
        auto it = m->lo_of.find(hi);
        if (it == m->lo_of.end()) return;
        free_owned(it->second);
        m->lo_of.erase(it);
    };
    auto pack_lo = [&](const bf16_t* W, const bf16_t* Wp, int N, int K) {   // the decode steps' packed copy of W's lo plane
        auto it = m->lo_of.find(W);
        if (it == m->lo_of.end()) return;
        bf16_t* lp = walloc<bf16_t>(m, (size_t)N * K);
        launch_pack_weight(it->second, lp, N, K, m->st);
        m->lo_of[Wp] = lp;
    };
    for (auto& L : m->llm) {
        launch_interleave_rows(L.gate_tmp, L.up_tmp, L.gu_w, F, D, m->st);
        if (m->lo_of.count(L.gate_tmp) || m->lo_of.count(L.up_tmp)) {
            for (bf16_t* t : {L.gate_tmp, L.up_tmp})
                if (!m->lo_of.count(t)) m->lo_of[t] = walloc<bf16_t>(m, (size_t)F * D, true);
            bf16_t* gu_lo = walloc<bf16_t>(m, (size_t)2 * F * D);
            launch_interleave_rows(m->lo_of[L.gate_tmp], m->lo_of[L.up_tmp], gu_lo, F, D, m->st);
            m->lo_of[L.gu_w] = gu_lo;
        }
        if (m->weight_format >= 1)
            for (const bf16_t* w : {L.qkv_w, L.o_w, L.gu_w, L.down_w}) drop_lo(w);
        decode_copy(L.qkv_w, 3 * D, D, L.qkv_p, L.qkv_s, L.qkv_q);
        decode_copy(L.o_w, D, D, L.o_p, L.o_s, L.o_q);
        decode_copy(L.gu_w, 2 * F, D, L.gu_p, L.gu_s, L.gu_q);
        decode_copy(L.down_w, D, F, L.down_p, L.down_s, L.down_q);
        if (m->weight_format == 0) {
            pack_lo(L.qkv_w, L.qkv_p, 3 * D, D);
            pack_lo(L.o_w, L.o_p, D, D);
            pack_lo(L.gu_w, L.gu_p, 2 * F, D);
            pack_lo(L.down_w, L.down_p, D, F);
        }
    }
    m->lm_head_p = walloc<bf16_t>(m, (size_t)V * D);
    launch_pack_weight(m->lm_head, m->lm_head_p, V, D, m->st);
    pack_lo(m->lm_head, m->lm_head_p, V, D);
    HIPCHK(hipStreamSynchronize(m->st));
    // gate/up staging copies (and their lo planes) are no longer needed
    for (auto& L : m->llm) {
        for (bf16_t** t : {&L.gate_tmp, &L.up_tmp}) {
            drop_lo(*t);
            free_owned(*t);
            *t = nullptr;
        }
    }
    // rope tables (LlamaRotaryEmbedding, [HF] llama/modeling_llama.py:73-127): inv_freq = theta^(-2i/hd) in fp32,
    // angle = pos * inv_freq in fp32, cos/sin in fp32
    const int half = m->hd / 2;
    std::vector<float> hc((size_t)c.max_positions * half), hs((size_t)c.max_positions * half);
    for (int i = 0; i < half; ++i) {
        const float inv = (float)(1.0 / pow((double)c.rope_theta, (double)(2 * i) / (double)m->hd));
        for (int p = 0; p < c.max_positions; ++p) {
            const float ang = (float)p * inv;
            hc[(size_t)p * half + i] = (float)cos((double)ang);
            hs[(size_t)p * half + i] = (float)sin((double)ang);
        }
    }
    m->rope_cos = walloc<float>(m, hc.size());
    m->rope_sin = walloc<float>(m, hs.size());
    HIPCHK(hipMemcpyAsync(m->rope_cos, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(m->rope_sin, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    m->stage.release();
    m->stage2.release();
    m->finalized = true;
    GUARD_END(m->ctx)
}

VC_API int vc_encode(vc_model* m, int modality, const float* pixels, int pixels_on_device, int B, float* out) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->finalized, VC_ERR_STATE, "vc_model_finalize() has not been called");
    REQUIRE(pixels && B >= 1 && modality >= 0 && modality <= 2, VC_ERR_INVALID, "bad encode arguments");
    REQUIRE(modality == VC_MOD_IMAGE || m->c.variant != VC_VARIANT_LLAVA, VC_ERR_INVALID, "llava has no seg/depth encoder");
    PixSet pix{{nullptr, nullptr, nullptr}, {0, 0, 0}};
    pix.p[modality] = pixels;
    pix.n[modality] = B;
    if (m->precision == 1) run_vit_and_adapters_strict(m, pix, pixels_on_device);
    else if (m->precision == 2) run_vit_and_adapters_split(m, pix, pixels_on_device);
    else run_vit_and_adapters(m, pix, pixels_on_device);
    if (out) {
        const size_t n = (size_t)m->feat_rows[modality] * m->c.hidden;
        if (m->precision) {
            HIPCHK(hipMemcpyAsync(out, m->s_feats.as<float>() + (size_t)m->feat_off[modality] * m->c.hidden, n * 4,
                                  hipMemcpyDeviceToHost, m->st));
        } else {
            m->v_patches.ensure(n * 4);
            launch_bf16_to_f32(m->feats.as<bf16_t>() + (size_t)m->feat_off[modality] * m->c.hidden, m->v_patches.as<float>(),
                               n, m->st);
            HIPCHK(hipMemcpyAsync(out, m->v_patches.p, n * 4, hipMemcpyDeviceToHost, m->st));
        }
    }
    HIPCHK(hipStreamSynchronize(m->st));
    GUARD_END(m->ctx)
}

/* CLIPVisionTower.forward + feature_select (multimodal_encoder/clip_encoder.py:29-51): the UN-projected tower output the
 * reference's encode_* functions hand to the adapters — hidden_states[select_layer] of N images, CLS dropped for 'patch'.
 * out [N, R, vit_hidden] fp32 on the host (R = patches, +1 with 'cls_patch'). */
VC_API int vc_vision_tower_forward(vc_model* m, const float* pixels, int pixels_on_device, int N, float* out) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->finalized, VC_ERR_STATE, "vc_model_finalize() has not been called");
    REQUIRE(pixels && out && N >= 1, VC_ERR_INVALID, "bad vision tower arguments");
    PixSet pix{{pixels, nullptr, nullptr}, {N, 0, 0}};
    int order[3], first[3];
    const int R = m->Tv - (m->c.vit_keep_cls ? 0 : 1);
    const size_t n = (size_t)N * R * m->c.vit_hidden;
    if (m->precision == 1) {
        run_vit_tower_strict(m, pix, pixels_on_device, order, first);
        HIPCHK(hipMemcpyAsync(out, m->s_sel.p, n * 4, hipMemcpyDeviceToHost, m->st));
    } else if (m->precision == 2) {
        run_vit_tower_split(m, pix, pixels_on_device, order, first);
        m->s_sel.ensure(n * 4);
        launch_select_rows_f32(m->v_x.as<float>(), m->s_sel.as<float>(), N, m->Tv, m->c.vit_keep_cls ? 0 : 1, m->c.vit_hidden, m->st);
        HIPCHK(hipMemcpyAsync(out, m->s_sel.p, n * 4, hipMemcpyDeviceToHost, m->st));
    } else {
        run_vit_tower(m, pix, pixels_on_device, order, first);
        m->v_patches.ensure(n * 4);
        launch_bf16_to_f32(m->v_sel.as<bf16_t>(), m->v_patches.as<float>(), n, m->st);
        HIPCHK(hipMemcpyAsync(out, m->v_patches.p, n * 4, hipMemcpyDeviceToHost, m->st));
    }
    HIPCHK(hipStreamSynchronize(m->st));
    GUARD_END(m->ctx)
}

/* images per sample for the NEXT vc_prefill* / vc_generate* call (one-shot): the reference's list / 5-D image form
 * (vcoder_ds_llava_arch.py:135-169), where sample b owns counts[b] images whose feature rows are spliced as ONE block at
 * its placeholder.  The pixel pointers of that call then hold sum(counts) images.  NULL = one image per sample. */
VC_API int vc_set_image_counts(vc_model* m, const int32_t* img, const int32_t* seg, const int32_t* depth, int B) {
    if (!m || B < 1) return VC_ERR_INVALID;
    const int32_t* src[3] = {img, seg, depth};
    for (int k = 0; k < 3; ++k) {
        m->img_counts[k].clear();
        if (!src[k]) continue;
        for (int b = 0; b < B; ++b) {
            if (src[k][b] < 1) {
                for (auto& v : m->img_counts) v.clear();
                m->ctx->err = "every sample needs at least one image per modality";
                return VC_ERR_INVALID;
            }
            m->img_counts[k].push_back(src[k][b]);
        }
    }
    return VC_OK;
}

/* output_hidden_states for the NEXT vc_prefill (one-shot): `out` (host, cap_floats floats) receives [(layers + 1), B, S, hidden]
 * fp32 — inputs_embeds, the residual stream behind every decoder layer, the last one after the final RMSNorm
 * ([HF] LlamaModel.forward all_hidden_states).  The buffer must stay valid until that vc_prefill returns. */
VC_API int vc_request_hidden_states(vc_model* m, float* out, size_t cap_floats) {
    if (!m) return VC_ERR_INVALID;
    m->hidden_out = out;
    m->hidden_cap = out ? cap_floats : 0;
    return VC_OK;
}

/* output_attentions for the NEXT vc_prefill (one-shot): `out` (host, cap_floats floats) receives [layers, B, heads, S, S] fp32,
 * the attention probabilities of every decoder layer (zeros above the diagonal and at hidden keys) */
VC_API int vc_request_attentions(vc_model* m, float* out, size_t cap_floats) {
    if (!m) return VC_ERR_INVALID;
    m->attn_out = out;
    m->attn_cap = out ? cap_floats : 0;
    return VC_OK;
}

/* attention_mask [B, T] (bytes, 0 = hidden) of the NEXT vc_prefill* / vc_generate* call (one-shot).  See include/vcoder_hip.h. */
VC_API int vc_set_attention_mask(vc_model* m, const uint8_t* mask, int B, int T) {
    if (!m || !mask || B < 1 || T < 1) return VC_ERR_INVALID;
    m->mask_next.assign(mask, mask + (size_t)B * T);
    m->mask_B = B;
    m->mask_T = T;
    return VC_OK;
}
/* the cached decode steps behind the current vc_prefill see every key again (what the reference's multimodal decode path does:
 * vcoder_ds_llava_arch.py:130-133 replaces the mask with ones) */
VC_API int vc_clear_attention_mask(vc_model* m) {
    if (!m) return VC_ERR_INVALID;
    m->kmask_in_decode = false;
    m->mask_next.clear();
    return VC_OK;
}

/* Token scores of the NEXT vc_prefill (labels [B, T] aligned with its ids) or vc_extend (labels [B, n] aligned with its tok), one-shot:
 * that call fills logprobs (host, [B, S] resp. [B, n]) with log p(label) of every labelled position and 0 elsewhere, and
 * spliced_labels (may be NULL) with the labels as the splice laid them out.  The labels are copied here; the output buffers must stay
 * valid until that call returns.  See include/vcoder_hip.h. */
VC_API int vc_request_token_scores(vc_model* m, const int64_t* labels, int B, int T, float* logprobs, int64_t* spliced_labels,
                                   size_t cap) {
    if (!m) return VC_ERR_INVALID;
    clear_score_request(m);
    if (!labels) return VC_OK;   // NULL cancels a pending request
    if (!logprobs || B < 1 || T < 1) {
        m->ctx->err = "vc_request_token_scores needs labels [B, T] and a logprobs buffer";
        return VC_ERR_INVALID;
    }
    m->score_labels.assign(labels, labels + (size_t)B * T);
    m->score_B = B;
    m->score_T = T;
    m->score_out = logprobs;
    m->score_labels_out = spliced_labels;
    m->score_cap = cap;
    return VC_OK;
}

/* Top-K alternatives of the scored positions: accompanies the pending vc_request_token_scores (one-shot with it).  The scored call fills
 * top_logprobs / top_ids (host, [B, S] or [B, n] x top_k, cap entries each) at the positions that carry a score; 0.0 / -1 elsewhere.
 * See include/vcoder_hip.h. */
VC_API int vc_request_top_logprobs(vc_model* m, int top_k, float* top_logprobs, int32_t* top_ids, size_t cap) {
    if (!m) return VC_ERR_INVALID;
    if (m->score_labels.empty()) {
        m->ctx->err = "vc_request_top_logprobs without a pending vc_request_token_scores";
        return VC_ERR_STATE;
    }
    if (top_k < 1 || top_k > VC_MAX_TOP_LOGPROBS || !top_logprobs || !top_ids) {
        m->ctx->err = "vc_request_top_logprobs needs top_k in 1 .. 32 and both output buffers";
        return VC_ERR_INVALID;
    }
    m->stk_k = top_k;
    m->stk_lp = top_logprobs;
    m->stk_ids = top_ids;
    m->stk_cap = cap;
    return VC_OK;
}

/* Per-token log-probs of the NEXT vc_generate* call (one-shot): log p(generated token) [B, max_new] and, with top_k > 0, the top_k most
 * likely tokens of every step [B, max_new, top_k], of the model's own next-token distribution.  token_logprobs == NULL cancels.  See
 * include/vcoder_hip.h. */
VC_API int vc_request_generate_logprobs(vc_model* m, int top_k, float* token_logprobs, float* top_logprobs, int32_t* top_ids,
                                        size_t cap_rows) {
    if (!m) return VC_ERR_INVALID;
    if (!token_logprobs) {
        clear_generate_logprobs_request(m);
        return VC_OK;
    }
    if (top_k < 0 || top_k > VC_MAX_TOP_LOGPROBS || (top_k > 0 && (!top_logprobs || !top_ids)) || cap_rows < 1) {
        m->ctx->err = "vc_request_generate_logprobs needs top_k in 0 .. 32, the top buffers iff top_k > 0, and cap_rows >= 1";
        return VC_ERR_INVALID;   // (a pending request stays as it was: nothing touched)
    }
    m->glp_k = top_k;
    m->glp_tok = token_logprobs;
    m->glp_top = top_k ? top_logprobs : nullptr;
    m->glp_ids = top_k ? top_ids : nullptr;
    m->glp_cap = cap_rows;
    return VC_OK;
}

/* Prompt-lookup speculation of the NEXT vc_generate* call (one-shot): k drafts per verify step from n-gram matches of at most
 * max_ngram ids in (lookup ids | prompt | generated).  k == 0 cancels.  See include/vcoder_hip.h. */
VC_API int vc_request_speculation(vc_model* m, int k, int max_ngram, const int32_t* lookup_ids, const int32_t* lookup_lens, int B) {
    if (!m) return VC_ERR_INVALID;
    if (k == 0) {
        clear_speculation_request(m);
        return VC_OK;
    }
    bool ok = k >= 1 && k <= 7 && max_ngram >= 1 && max_ngram <= 4 && (lookup_ids == nullptr) == (lookup_lens == nullptr) &&
              (lookup_ids == nullptr || (B >= 1 && B <= VC_MAX_ROWS));
    int stride = 0;
    for (int b = 0; ok && lookup_ids && b < B; ++b) {
        ok = lookup_lens[b] >= 0 && lookup_lens[b] <= m->c.max_positions;
        stride = std::max(stride, (int)lookup_lens[b]);
    }
    if (!ok) {
        m->ctx->err = "vc_request_speculation needs k in 1 .. 7, max_ngram in 1 .. 4 and, with lookup ids, their lengths (0 .. "
                      "max_position_embeddings each) for 1 .. 16 sequences";
        return VC_ERR_INVALID;   // (a pending request stays as it was: nothing touched)
    }
    clear_speculation_request(m);
    m->spec_k = k;
    m->spec_ngram = max_ngram;
    if (lookup_ids) {   // ragged in, [B][longest] here
        m->spec_B = B;
        m->spec_lookup_stride = stride;
        m->spec_lookup.assign((size_t)B * std::max(stride, 1), 0);
        m->spec_lookup_len.assign(lookup_lens, lookup_lens + B);
        size_t off = 0;
        for (int b = 0; b < B; ++b) {
            std::copy(lookup_ids + off, lookup_ids + off + lookup_lens[b], m->spec_lookup.begin() + (size_t)b * std::max(stride, 1));
            off += lookup_lens[b];
        }
    }
    return VC_OK;
}
/* The selections a pending vc_request_speculation is served for: 0 greedy calls without logits processors, != 0 sampled calls and
 * calls with processors as well.  Travels with the request.  See include/vcoder_hip.h. */
VC_API int vc_request_speculation_selection(vc_model* m, int any) {
    if (!m) return VC_ERR_INVALID;
    if (m->spec_k == 0) {
        m->ctx->err = "vc_request_speculation_selection: no vc_request_speculation is pending";
        return VC_ERR_STATE;
    }
    m->spec_any = any != 0;
    return VC_OK;
}
/* the counters of the last vc_generate* call if it speculated: out [B][4] = steps, tokens emitted, drafts proposed, drafts accepted per
 * sequence; VC_OK, or VC_ERR_STATE ("not speculated") */
VC_API int vc_last_speculation(vc_model* m, int32_t* out, int B) {
    if (!m || !out) return VC_ERR_INVALID;
    if (!m->spec_last || (size_t)B * 4 != m->spec_counters.size()) {
        m->ctx->err = "the last generate call of this session was not speculated";
        return VC_ERR_STATE;
    }
    std::copy(m->spec_counters.begin(), m->spec_counters.end(), out);
    return VC_OK;
}

/* Fan-out of the NEXT vc_generate call (one-shot): n returned sequences per prompt, rows b n + j.  n <= 1 cancels.  See
 * include/vcoder_hip.h. */
VC_API int vc_request_fanout(vc_model* m, int n) {
    if (!m) return VC_ERR_INVALID;
    if (n < -VC_MAX_ROWS || n > VC_MAX_ROWS) {
        m->ctx->err = "vc_request_fanout needs |n| <= 16 (batch x n rows: at most 16 sequences per GPU replica)";
        return VC_ERR_INVALID;
    }
    m->fan_n = abs(n) <= 1 ? 0 : abs(n);
    m->fan_share = n > 0;   // n < -1: |n| sequences per prompt with the prompts repeated (the request is not served)
    return VC_OK;
}
/* what the last vc_generate of this session made of a fan-out request: out = {n, shared (1: one prefill, the fan-out attention; 0:
 * the prompts were expanded), prompt rows prefilled}; VC_OK, or VC_ERR_STATE (no request) */
VC_API int vc_last_fanout(vc_model* m, int32_t* out) {
    if (!m || !out) return VC_ERR_INVALID;
    if (!m->fan_last) {
        m->ctx->err = "the last generate call of this session had no fan-out request";
        return VC_ERR_STATE;
    }
    out[0] = m->fan_last_n;
    out[1] = m->fan_last_shared ? 1 : 0;
    out[2] = m->fan_last_B;
    return VC_OK;
}

/* Logits processors of the NEXT vc_generate* call (one-shot): repetition penalty, no-repeat n-gram, bad words, minimum new tokens,
 * applied on the device in front of every selection.  p == NULL cancels.  See include/vcoder_hip.h. */
VC_API int vc_request_logits_processors(vc_model* m, const vc_logits_processors* p) {
    if (!m) return VC_ERR_INVALID;
    if (!p) {
        clear_logits_processors_request(m);
        return VC_OK;
    }
    // (a refusal leaves a pending request as it was: nothing touched)
    if (!(p->repetition_penalty > 0.f) || !std::isfinite(p->repetition_penalty)) {
        m->ctx->err = "vc_request_logits_processors: repetition_penalty must be a finite value above 0";
        return VC_ERR_INVALID;
    }
    if (p->no_repeat_ngram_size < 0 || p->min_new_tokens < 0) {
        m->ctx->err = "vc_request_logits_processors: no_repeat_ngram_size and min_new_tokens must not be negative";
        return VC_ERR_INVALID;
    }
    if (p->n_bad_words < 0 || p->n_bad_words > VC_MAX_BAD_WORDS || (p->n_bad_words > 0 && (!p->bad_words_ids || !p->bad_words_lens)) ||
        p->n_eos_extra < 0 || p->n_eos_extra > VC_MAX_EOS_EXTRA || (p->n_eos_extra > 0 && !p->eos_extra)) {
        m->ctx->err = "vc_request_logits_processors: at most 32 bad-word sequences and 8 further EOS ids";
        return VC_ERR_INVALID;
    }
    for (int q = 0; q < p->n_bad_words; ++q)
        if (p->bad_words_lens[q] < 1 || p->bad_words_lens[q] > VC_MAX_BAD_WORD_LEN) {
            m->ctx->err = "vc_request_logits_processors: a bad-word sequence holds 1 .. 8 ids";
            return VC_ERR_INVALID;
        }
    m->gproc = true;
    m->gproc_penalty = p->repetition_penalty;
    m->gproc_ngram = p->no_repeat_ngram_size;
    m->gproc_minnew = p->min_new_tokens;
    m->gproc_nbad = p->n_bad_words;
    m->gproc_neos = p->n_eos_extra;
    for (int e = 0; e < p->n_eos_extra; ++e) m->gproc_eos[e] = p->eos_extra[e];
    m->gproc_bad.assign((size_t)VC_MAX_BAD_WORDS * (1 + VC_MAX_BAD_WORD_LEN), 0);
    for (int q = 0, off = 0; q < p->n_bad_words; ++q) {
        int* e = m->gproc_bad.data() + (size_t)q * (1 + VC_MAX_BAD_WORD_LEN);
        e[0] = p->bad_words_lens[q];
        for (int j = 0; j < e[0]; ++j) e[1 + j] = p->bad_words_ids[off + j];
        off += e[0];
    }
    return VC_OK;
}

/* Token automaton of the NEXT vc_generate call (one-shot): constrained decoding on the device, behind the logits processors.
 * a == NULL cancels.  See include/vcoder_hip.h. */
VC_API int vc_request_constraint(vc_model* m, const vc_token_automaton* a) {
    if (!m) return VC_ERR_INVALID;
    if (!a) {
        clear_constraint_request(m);
        return VC_OK;
    }
    // (a refusal leaves a pending request as it was: nothing touched)
    auto refuse = [&](const char* why) {
        m->ctx->err = std::string("vc_request_constraint: ") + why;
        return VC_ERR_INVALID;
    };
    const int S = a->n_states, E = a->n_edges;
    if (S < 1 || S > VC_MAX_AUTOMATON_STATES || E < 0 || E > VC_MAX_AUTOMATON_EDGES) return refuse("1 .. 65536 states and at most 1 << 20 edges");
    if (!a->state_off || !a->default_next || (E > 0 && (!a->edge_tok || !a->edge_next))) return refuse("a table is missing");
    if (a->state_off[0] != 0 || a->state_off[S] != E) return refuse("state_off must run from 0 to n_edges");
    for (int s = 0; s < S; ++s) {
        const int e0 = a->state_off[s], e1 = a->state_off[s + 1];
        if (e0 > e1 || e1 > E) return refuse("state_off must not fall");
        for (int e = e0 + 1; e < e1; ++e)
            if (a->edge_tok[e - 1] >= a->edge_tok[e]) return refuse("the edge ids of a state must be ascending and unique");
        if (a->default_next[s] < -1 || a->default_next[s] >= S) return refuse("default_next outside [-1, n_states)");
    }
    for (int e = 0; e < E; ++e)
        if (a->edge_next[e] < -1 || a->edge_next[e] >= S) return refuse("edge_next outside [-1, n_states)");
    {   // every state reachable from 0 allows at least one token
        std::vector<char> seen((size_t)S, 0);
        std::vector<int> todo{0};
        seen[0] = 1;
        while (!todo.empty()) {
            const int s = todo.back();
            todo.pop_back();
            const int e0 = a->state_off[s], e1 = a->state_off[s + 1];
            if (e0 == e1 && a->default_next[s] < 0) return refuse("a reachable state allows no token");
            auto visit = [&](int t) {
                if (t >= 0 && !seen[t]) {
                    seen[t] = 1;
                    todo.push_back(t);
                }
            };
            for (int e = e0; e < e1; ++e) visit(a->edge_next[e]);
            visit(a->default_next[s]);
        }
    }
    m->gcn_tab.resize((size_t)2 * S + 1 + 2 * (size_t)E);
    int* t = m->gcn_tab.data();
    std::copy(a->state_off, a->state_off + S + 1, t);
    if (E > 0) {
        std::copy(a->edge_tok, a->edge_tok + E, t + S + 1);
        std::copy(a->edge_next, a->edge_next + E, t + S + 1 + E);
    }
    std::copy(a->default_next, a->default_next + S, t + S + 1 + 2 * (size_t)E);
    m->gcn_S = S;
    m->gcn_E = E;
    return VC_OK;
}

/* KV-cache slots the next vc_prefill keeps free behind the prompt for vc_decode_step (default 64; clamped to
 * max_position_embeddings).  A decode loop that outruns the reserve still works — the cache grows, at the cost of a copy. */
VC_API int vc_model_reserve_decode(vc_model* m, int max_new_tokens) {
    if (!m || max_new_tokens < 0) return VC_ERR_INVALID;
    m->reserve_new = max_new_tokens;
    return VC_OK;
}

/* Classifier-free guidance of the NEXT vc_generate / vc_prefill call (one-shot).  neg_ids == NULL cancels.  See
 * include/vcoder_hip.h. */
VC_API int vc_request_guidance(vc_model* m, float scale, const int64_t* neg_ids, int B, int Tn, const float* neg_img,
                               const float* neg_seg, const float* neg_depth, int pixels_on_device) {
    if (!m) return VC_ERR_INVALID;
    if (!neg_ids) {
        clear_guidance_request(m);
        return VC_OK;
    }
    // (a refusal leaves a pending request as it was: nothing touched)
    if (!std::isfinite(scale)) {
        m->ctx->err = "vc_request_guidance: the scale must be finite";
        return VC_ERR_INVALID;
    }
    if (B < 1 || 2 * B > VC_MAX_ROWS || Tn < 1) {
        m->ctx->err = "vc_request_guidance needs 1 <= B <= 8 negative prompts (2 B rows: at most 16 per GPU replica) of at least one id";
        return VC_ERR_INVALID;
    }
    m->gd_on = true;
    m->gd_scale = scale;
    m->gd_ids.assign(neg_ids, neg_ids + (size_t)B * Tn);
    m->gd_B = B;
    m->gd_T = Tn;
    m->gd_px[0] = neg_img;
    m->gd_px[1] = neg_img ? neg_seg : nullptr;
    m->gd_px[2] = neg_img ? neg_depth : nullptr;
    m->gd_px_on_dev = pixels_on_device;
    return VC_OK;
}
/* what the last vc_generate / vc_prefill of this session made of a guidance request: out = {served (1), conditional rows B, spliced
 * length of the prompts, spliced length of the negative prompts}; VC_OK, or VC_ERR_STATE (no request) */
VC_API int vc_last_guidance(vc_model* m, int32_t* out) {
    if (!m || !out) return VC_ERR_INVALID;
    if (!m->gd_last) {
        m->ctx->err = "the last generate / prefill call of this session had no guidance request";
        return VC_ERR_STATE;
    }
    out[0] = 1;
    out[1] = m->gd_last_B;
    out[2] = m->gd_last_Sc;
    out[3] = m->gd_last_Sn;
    return VC_OK;
}

/* The further warpers of the NEXT vc_generate call (one-shot): min_p, typical_p, epsilon_cutoff, eta_cutoff behind temperature /
 * top-k / top-p of a sampled call.  See include/vcoder_hip.h. */
VC_API int vc_request_sampling_warpers(vc_model* m, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff) {
    if (!m) return VC_ERR_INVALID;
    // (a refusal leaves a pending request as it was: nothing touched)
    auto refuse = [&](const char* why) {
        m->ctx->err = std::string("vc_request_sampling_warpers: ") + why;
        return VC_ERR_INVALID;
    };
    if (!(min_p >= 0.f && min_p <= 1.f)) return refuse("min_p must be in [0, 1]");
    if (!(typical_p > 0.f) || !std::isfinite(typical_p)) return refuse("typical_p must be positive (>= 1: off)");
    if (!(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f)) return refuse("epsilon_cutoff must be in [0, 1)");
    if (!(eta_cutoff >= 0.f && eta_cutoff < 1.f)) return refuse("eta_cutoff must be in [0, 1)");
    m->warp_min_p = min_p;
    m->warp_typical = typical_p < 1.f ? typical_p : 0.f;
    m->warp_eps = epsilon_cutoff;
    m->warp_eta = eta_cutoff;
    return VC_OK;
}

namespace {
void guided_prefill(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth, int on_dev,
                    int has_mask, float* logits_last, int* S_out);   // engine_pool.inc
}

VC_API int vc_prefill(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                      const float* depth, int pixels_on_device, int has_attention_mask, float* logits_last,
                      float* logits_all, int* S_out) {
    if (!m) return VC_ERR_INVALID;
    OneShotReset one_shot{m};
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    m->gd_last = false;
    if (m->gd_on) {
        // vc_request_guidance: the loop of 2 B rows a host loop steps with vc_decode_step over 2 B tokens; every refusal comes before
        // anything of the session is touched
        REQUIRE(m->score_labels.empty() && !logits_all && !m->hidden_out && !m->attn_out, VC_ERR_STATE,
                "a guided vc_prefill returns its 2 B last-row logits only (no labels, all-row logits, hidden states or attentions)");
        REQUIRE(m->gd_B == B, VC_ERR_INVALID, "negative prompts given for %d sequences, batch is %d", m->gd_B, B);
        guided_prefill(m, ids, B, T, img, seg, depth, pixels_on_device, has_attention_mask, logits_last, S_out);
        return VC_OK;
    }
    if (!m->score_labels.empty()) {
        // vc_request_token_scores: a scored prefill is refused while the session's cache and position are still what they were — the
        // shape here, the label range and the capacity behind the splice plan in do_prefill, which drops the position only then
        REQUIRE(ids && m->score_B == B && m->score_T == T, VC_ERR_INVALID, "labels are [%d, %d], input_ids [%d, %d]", m->score_B,
                m->score_T, B, T);
        m->score_on = true;
    } else {
        m->cur_pos = -1;
    }
    do_prefill(m, ids, B, T, img, seg, depth, pixels_on_device, has_attention_mask, -std::max(m->reserve_new, 1), true, S_out);
    ensure_out_ids(m, B, 1);
    finish_prefill(m, session_kv(m), logits_all);
    // a vc_decode_step loop behind this prefill keeps the hidden keys hidden (a caller that carries its attention_mask through
    // the steps: forward() without images); vc_clear_attention_mask() gives the steps the all-ones mask the reference's
    // multimodal decode path builds (vcoder_ds_llava_arch.py:130-133)
    m->kmask_in_decode = m->has_kmask;
    // greedy choice of the prefill logits, so that vc_decode_step(tok = NULL) continues the sequence: nothing is recorded
    // (max_new 0), no EOS bookkeeping, the position stays at S
    GenParams g;
    arm_session_rows(m, g, nullptr);
    const LoopView v = session_view(m);
    enqueue_selection(m, v, v.logits, B, 0);
    HIPCHK(hipStreamSynchronize(m->st));
    if (logits_last) {
        HIPCHK(hipMemcpyAsync(logits_last, m->logits.p, (size_t)B * m->c.vocab * 4, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
    }
    GUARD_END(m->ctx)
}

/* splice only (no decoder layers): inputs_embeds [B,S,hidden] fp32 to host.  Used by the parity tests of a7. */
VC_API int vc_prefill_embeds_only(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                                  const float* depth, int pixels_on_device, int has_attention_mask, float* out_host,
                                  int* S_out) {
    if (!m) return VC_ERR_INVALID;
    OneShotReset one_shot{m};
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    m->cur_pos = -1;
    int S = 0;
    do_prefill(m, ids, B, T, img, seg, depth, pixels_on_device, has_attention_mask, -1, true, &S);
    if (S_out) *S_out = S;
    if (out_host) {
        HIPCHK(hipMemcpyAsync(out_host, m->x.p, (size_t)B * S * m->c.hidden * 4, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
    }
    GUARD_END(m->ctx)
}

/* The spliced length S a vc_prefill* / vc_generate* call with these arguments would produce — the splice plan alone (ids,
 * which modalities are present, the per-sample image counts of vc_set_image_counts, is_depth_zero of the depth pixels): no
 * tower pass, no cache or mask state touched.  Same errors as the real call's plan (IndexError / quirk 6). */
VC_API int vc_plan_spliced_len(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                               const float* depth, int pixels_on_device, int has_attention_mask, int* S_out) {
    if (!m) return VC_ERR_INVALID;
    struct Reset {
        vc_model* m;
        ~Reset() {
            m->plan_only = false;
            for (auto& v : m->img_counts) v.clear();
        }
    } reset{m};
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    m->plan_only = true;
    do_prefill(m, ids, B, T, img, seg, depth, pixels_on_device, has_attention_mask, -1, false, S_out);
    GUARD_END(m->ctx)
}

/* Parity diagnostic (tests/: per-layer teacher forcing): decoder layers [l0, l1) of a PREFILL applied to a caller-supplied
 * residual stream x_in [B, S, hidden] (fp32, host) at positions 0..S-1, in the model's weight format and precision mode;
 * x_out receives the residual stream behind layer l1 - 1.  Feeding every layer the ORACLE's input isolates that layer's
 * arithmetic: quantisation noise of the layers in front cannot compound.  Uses the session's own KV cache. */
VC_API int vc_debug_prefill_layers(vc_model* m, int l0, int l1, const float* x_in, int B, int S, float* x_out) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->finalized, VC_ERR_STATE, "vc_model_finalize() has not been called");
    REQUIRE(x_in && x_out && B >= 1 && B <= VC_MAX_ROWS && S >= 1 && l0 >= 0 && l1 > l0 && l1 <= m->c.layers, VC_ERR_INVALID,
            "bad layer range / shape");
    m->cur_pos = -1;
    m->has_kmask = m->kmask_in_decode = false;   // a diagnostic pass over caller-supplied rows: no key mask of an earlier prefill
    ensure_llm(m, B, S + 1);
    const size_t n = (size_t)B * S * m->c.hidden;
    HIPCHK(hipMemcpyAsync(m->x.p, x_in, n * 4, hipMemcpyHostToDevice, m->st));
    if (m->precision == 1) {
        ensure_strict(m, B, m->capS);
        REQUIRE(l0 == 0 && l1 == m->c.layers, VC_ERR_INVALID, "strict mode runs the whole stack");
        run_llm_layers_strict(m, m->x.as<float>(), B, S, nullptr, true);
    } else if (m->precision == 2) {
        run_prefill_layers_split(m, session_kv(m), B, S, l0, l1);
    } else {
        run_prefill_layers(m, session_kv(m), B, S, l0, l1);
    }
    HIPCHK(hipMemcpyAsync(x_out, m->x.p, n * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    GUARD_END(m->ctx)
}

/* Captures of a decode step this session has performed so far (the session's own loop: vc_decode_step, vc_generate* with the pool
 * off, vc_generate_beam; not the pool's).  A test hook: a call that replays a captured step adds 0. */
VC_API int vc_debug_step_captures(vc_model* m) { return m ? m->step_captures : VC_ERR_INVALID; }

/* Beam search support: the KV rows of the session's current loop are permuted, row r <- old row src_rows[r] (live prefix only) —
 * `past_key_values` reordered by beam_idx ([HF] generation/utils.py: _reorder_cache after every beam step). */
VC_API int vc_reorder_cache(vc_model* m, const int32_t* src_rows, int B) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->cur_pos >= 0, VC_ERR_STATE, "vc_reorder_cache before vc_prefill");
    REQUIRE(!m->gd_pair, VC_ERR_STATE, "vc_reorder_cache behind a guided vc_prefill: its rows are pairs at different positions");
    REQUIRE(src_rows && B == m->curB, VC_ERR_INVALID, "beam_idx must have one entry per row of the current batch (%d)", m->curB);
    bool identity = true;
    for (int b = 0; b < B; ++b) {
        REQUIRE(src_rows[b] >= 0 && src_rows[b] < B, VC_ERR_INDEX, "beam index %d out of range", src_rows[b]);
        identity = identity && src_rows[b] == b;
    }
    if (!identity) {
        const vc_model_cfg& c = m->c;
        const int live = m->cur_pos, H = c.heads;
        const bool strict = m->precision == 1;
        const size_t es = strict ? 4 : (size_t)m->kv_es;
        const int capS = strict ? m->s_capS : m->capS, capB = strict ? m->s_capB : m->capB;
        const size_t cap_row = (size_t)capS * m->hd * es, live_row = (size_t)live * m->hd * es;
        m->stage.ensure((size_t)B * H * live_row);
        m->stage2.ensure((size_t)B * 4);
        HIPCHK(hipMemcpyAsync(m->stage2.p, src_rows, (size_t)B * 4, hipMemcpyHostToDevice, m->st));
        char* kb = reinterpret_cast<char*>(strict ? m->s_kc.p : m->kc.p);
        char* vb = reinterpret_cast<char*>(strict ? m->s_vc.p : m->vc.p);
        for (int l = 0; l < c.layers; ++l) {
            const size_t off = (size_t)l * capB * H * cap_row;
            launch_kv_permute(kb + off, m->stage.p, m->stage2.as<int>(), B, H, cap_row, live_row, m->st);
            launch_kv_permute(vb + off, m->stage.p, m->stage2.as<int>(), B, H, cap_row, live_row, m->st);
        }
        HIPCHK(hipStreamSynchronize(m->st));
    }
    GUARD_END(m->ctx)
}

/* The session's loop steps back to position P: cached rows >= P are dead, nothing is copied.  See include/vcoder_hip.h. */
VC_API int vc_rewind(vc_model* m, int P) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->cur_pos >= 0, VC_ERR_STATE, "vc_rewind before vc_prefill");
    REQUIRE(!m->gd_pair, VC_ERR_STATE, "vc_rewind behind a guided vc_prefill: its rows stand at different positions");
    REQUIRE(P >= m->curS && P <= m->cur_pos, VC_ERR_INVALID, "vc_rewind to %d: the prompt ends at %d, the loop stands at %d", P,
            m->curS, m->cur_pos);
    if (P != m->cur_pos) {
        const std::vector<int> pos(m->curB, P);   // RS_POS of every row (the hidden-key mask of the prefill stays in force)
        HIPCHK(hipMemcpy2DAsync(m->rows.as<int>() + RS_POS, (size_t)RS_STRIDE * 4, pos.data(), 4, 4, m->curB, hipMemcpyHostToDevice,
                                m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        m->cur_pos = P;
        m->tok_stale = true;
    }
    GUARD_END(m->ctx)
}

// one cached step of the session's loop (vc_decode_step; vc_extend in precision modes "strict" / "split")
void decode_step_impl(vc_model* m, const int32_t* tok, float* logits, int32_t* next_tok) {
    REQUIRE(!(m->cur_pos < 0 && m->spec_closed), VC_ERR_STATE,
            "vc_decode_step behind a speculated generate: its rows stand at different positions (prefill again)");
    REQUIRE(!(m->cur_pos < 0 && m->fan_closed), VC_ERR_STATE,
            "vc_decode_step behind a fan-out generate: a cache row no longer holds one sequence (prefill again)");
    REQUIRE(!(m->cur_pos < 0 && m->gd_closed), VC_ERR_STATE,
            "vc_decode_step behind a guided generate: its rows stand at different positions (prefill again)");
    REQUIRE(m->cur_pos >= 0, VC_ERR_STATE, "vc_decode_step before vc_prefill");
    REQUIRE(!m->gd_pair || !(m->hidden_out || m->attn_out), VC_ERR_STATE,
            "hidden states / attentions of a step behind a guided vc_prefill: its rows stand at different positions");
    REQUIRE(tok || !m->tok_stale, VC_ERR_STATE,
            "vc_decode_step(tok = NULL) after vc_rewind: the token selected on the device belongs to the rows that were dropped");
    if (m->cur_pos + 1 > m->capS) grow_kv(m, m->cur_pos + 1);
    const int B = m->curB;
    const LoopView v = session_view(m);   // the plain step, whatever call ran before
    if (tok) {
        for (int b = 0; b < B; ++b)
            REQUIRE(tok[b] >= 0 && tok[b] < m->c.vocab, VC_ERR_INDEX, "index out of range in self (token id %d)", tok[b]);
        HIPCHK(hipMemcpyAsync(m->next_tok.p, tok, B * 4, hipMemcpyHostToDevice, m->st));
        launch_embed_tokens_ssq(m->next_tok.as<int>(), m->embed, m->x_dec.as<float>(), m->ssq.as<float>(), m->llm[0].in_norm,
                                m->xg_dec.as<bf16_t>(), B, m->c.hidden, m->npart, m->st, v.split_G,
                                m->precision ? lo_plane(m, m->embed) : nullptr);
    }
    struct StepRequests {   // one-shot, also when the step fails
        vc_model* m;
        ~StepRequests() {
            m->hidden_out = nullptr;
            m->attn_out = nullptr;
            m->hidden_cap = m->attn_cap = 0;
            clear_generate_logprobs_request(m);
            clear_logits_processors_request(m);
        }
    } step_requests{m};
    if (m->precision == 1) {
        enqueue_decode_step_strict(m, v, B);
    } else if (m->hidden_out || m->attn_out) {
        enqueue_decode_step(m, v, B, m->cur_pos);
    } else {
        HIPCHK(hipGraphLaunch(step_graph(m, STEP_PLAIN, v, B), m->st));
    }
    m->cur_pos += 1;
    m->tok_stale = false;
    if (logits) HIPCHK(hipMemcpyAsync(logits, m->logits.p, (size_t)B * m->c.vocab * 4, hipMemcpyDeviceToHost, m->st));
    if (next_tok) HIPCHK(hipMemcpyAsync(next_tok, m->next_tok.p, B * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
}

VC_API int vc_decode_step(vc_model* m, const int32_t* tok, float* logits, int32_t* next_tok) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    decode_step_impl(m, tok, logits, next_tok);
    GUARD_END(m->ctx)
}

/* Multi-token continuation of the session's cached rows: tok [B, n] at positions P .. P+n-1 (P = the loop's position).  See
 * include/vcoder_hip.h. */
VC_API int vc_extend(vc_model* m, const int32_t* tok, int B, int n, float* logits_all, float* logits_last) {
    if (!m) return VC_ERR_INVALID;
    float* const hidden_req = m->hidden_out;
    float* const attn_req = m->attn_out;
    const size_t hidden_cap = m->hidden_cap, attn_cap = m->attn_cap;
    struct Requests {   // one-shot, also when the call fails
        vc_model* m;
        ~Requests() {
            m->hidden_out = nullptr;
            m->attn_out = nullptr;
            m->hidden_cap = m->attn_cap = 0;
            clear_score_request(m);
            clear_generate_logprobs_request(m);
            clear_logits_processors_request(m);
        }
    } requests{m};
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    const vc_model_cfg& c = m->c;
    // every check before anything is enqueued: a refused call leaves the cache and the loop's state as they were
    REQUIRE(!(m->cur_pos < 0 && m->spec_closed), VC_ERR_STATE,
            "vc_extend behind a speculated generate: its rows stand at different positions (prefill again)");
    REQUIRE(!(m->cur_pos < 0 && m->fan_closed), VC_ERR_STATE,
            "vc_extend behind a fan-out generate: a cache row no longer holds one sequence (prefill again)");
    REQUIRE(!(m->cur_pos < 0 && m->gd_closed), VC_ERR_STATE,
            "vc_extend behind a guided generate: its rows stand at different positions (prefill again)");
    REQUIRE(m->cur_pos >= 0, VC_ERR_STATE, "vc_extend before vc_prefill");
    REQUIRE(!m->gd_pair, VC_ERR_STATE, "vc_extend behind a guided vc_prefill: its rows stand at different positions");
    REQUIRE(tok && n >= 1, VC_ERR_INVALID, "vc_extend needs n >= 1 tokens per row");
    REQUIRE(B == m->curB, VC_ERR_INVALID, "vc_extend: %d rows given, the session's loop has %d", B, m->curB);
    for (size_t i = 0; i < (size_t)B * n; ++i)
        REQUIRE(tok[i] >= 0 && tok[i] < c.vocab, VC_ERR_INDEX, "index out of range in self (token id %d)", tok[i]);
    const int P = m->cur_pos, V = c.vocab, L = c.layers;
    REQUIRE(P + n <= c.max_positions / 64 * 64, VC_ERR_STATE, "KV cache full: position %d exceeds max_position_embeddings=%d",
            P + n, c.max_positions);
    REQUIRE(!attn_req || P + n <= 4096, VC_ERR_INVALID, "output_attentions: at most 4096 positions");
    REQUIRE(!hidden_req || hidden_cap >= (size_t)(L + 1) * B * n * c.hidden, VC_ERR_INVALID, "hidden-state buffer too small");
    REQUIRE(!attn_req || attn_cap >= (size_t)L * B * c.heads * n * (P + n), VC_ERR_INVALID, "attention buffer too small");
    const bool scored = !m->score_labels.empty();   // vc_request_token_scores: labels [B, n] aligned with tok
    const int64_t* labels = m->score_labels.data();
    if (scored) {
        REQUIRE(m->score_B == B && m->score_T == n, VC_ERR_INVALID, "labels are [%d, %d], the tokens [%d, %d]", m->score_B, m->score_T,
                B, n);
        REQUIRE(m->score_cap >= (size_t)B * n, VC_ERR_INVALID, "token-score buffers hold %zu elements, the call yields [%d, %d]",
                m->score_cap, B, n);
        REQUIRE(!m->stk_k || m->stk_cap >= (size_t)B * n * m->stk_k, VC_ERR_INVALID,
                "top-logprob buffers hold %zu entries, the call yields [%d, %d, %d]", m->stk_cap, B, n, m->stk_k);
        for (size_t i = 0; i < (size_t)B * n; ++i)
            REQUIRE(labels[i] == IGNORE_INDEX || (labels[i] >= 0 && labels[i] < V), VC_ERR_INDEX, "Target %lld is out of bounds.",
                    (long long)labels[i]);
    }
    if (m->precision != 0) {
        // "strict" / "split": n cached steps of the session's loop (the same launches as n vc_decode_step calls); the per-step
        // diagnostics are gathered into the [.., B, n, ..] layouts of the call
        const size_t D = c.hidden, H = c.heads;
        std::vector<int32_t> col(B);
        std::vector<float> step_lg((size_t)B * V), hs, at;
        if (attn_req) std::fill(attn_req, attn_req + (size_t)L * B * H * n * (P + n), 0.f);
        // scores: step t's logits [B, V] against label t + 1 (unlabelled rows against token 0, dropped below); one copy at the end
        std::vector<int> tgt((size_t)std::max(n - 1, 1) * B, 0);
        if (scored && n > 1) {
            for (int t = 0; t + 1 < n; ++t)
                for (int b = 0; b < B; ++b)
                    if (labels[(size_t)b * n + t + 1] != IGNORE_INDEX) tgt[(size_t)t * B + b] = (int)labels[(size_t)b * n + t + 1];
            m->sc_idx.ensure(tgt.size() * 4);
            m->sc_lp.ensure(tgt.size() * 4);
            ensure_score_top(m, tgt.size());
            HIPCHK(hipMemcpyAsync(m->sc_idx.p, tgt.data(), tgt.size() * 4, hipMemcpyHostToDevice, m->st));
        }
        for (int t = 0; t < n; ++t) {
            for (int b = 0; b < B; ++b) col[b] = tok[(size_t)b * n + t];
            if (hidden_req) {
                hs.assign((L + 1) * B * D, 0.f);
                m->hidden_out = hs.data();
                m->hidden_cap = hs.size();
            }
            if (attn_req) {
                at.assign((size_t)L * B * H * (P + t + 1), 0.f);
                m->attn_out = at.data();
                m->attn_cap = at.size();
            }
            decode_step_impl(m, col.data(), step_lg.data(), nullptr);
            if (scored && t + 1 < n) {
                launch_token_logprob(m->logits.as<float>(), V, m->sc_idx.as<int>() + (size_t)t * B, m->sc_lp.as<float>() + (size_t)t * B, B,
                                     V, m->st);
                score_top_rows(m, m->logits.as<float>(), (size_t)t * B, B);
            }
            if (logits_all)
                for (int b = 0; b < B; ++b) memcpy(logits_all + ((size_t)b * n + t) * V, step_lg.data() + (size_t)b * V, (size_t)V * 4);
            if (hidden_req)
                for (size_t e = 0; e < (size_t)(L + 1) * B; ++e)
                    memcpy(hidden_req + (e * n + t) * D, hs.data() + e * D, D * 4);
            if (attn_req)
                for (size_t e = 0; e < (size_t)L * B * H; ++e)
                    memcpy(attn_req + (e * n + t) * (P + n), at.data() + e * (P + t + 1), (size_t)(P + t + 1) * 4);
        }
        if (logits_last) memcpy(logits_last, step_lg.data(), step_lg.size() * 4);
        if (scored) {
            std::fill(m->score_out, m->score_out + (size_t)B * n, 0.f);
            top_fill(m, (size_t)B * n);
            if (n > 1) {
                std::vector<float> lp((size_t)(n - 1) * B);
                TopHost top;
                HIPCHK(hipMemcpyAsync(lp.data(), m->sc_lp.p, lp.size() * 4, hipMemcpyDeviceToHost, m->st));
                top.fetch(m, lp.size());
                HIPCHK(hipStreamSynchronize(m->st));
                for (int t = 0; t + 1 < n; ++t)
                    for (int b = 0; b < B; ++b)
                        if (labels[(size_t)b * n + t + 1] != IGNORE_INDEX) {
                            m->score_out[(size_t)b * n + t + 1] = lp[(size_t)t * B + b];
                            top.scatter(m, (size_t)t * B + b, (size_t)b * n + t + 1);
                        }
            }
            if (m->score_labels_out) std::copy(labels, labels + (size_t)B * n, m->score_labels_out);
        }
        return VC_OK;
    }
    if (P + n > m->capS) grow_kv(m, P + n);
    m->hidden_out = hidden_req;
    m->hidden_cap = hidden_cap;
    m->attn_out = attn_req;
    m->attn_cap = attn_cap;
    m->ext_tok.ensure((size_t)B * n * 4);
    HIPCHK(hipMemcpyAsync(m->ext_tok.p, tok, (size_t)B * n * 4, hipMemcpyHostToDevice, m->st));
    const bool all_rows = logits_all != nullptr || B * n <= EXTEND_GEMV_ROWS;
    run_extend(m, m->ext_tok.as<int>(), B, n, logits_all != nullptr);
    if (scored) {   // (the lm_head ran over every row: score them in place; otherwise the labelled rows through the score path)
        if (all_rows) score_logits_rows(m, m->logits_all.as<float>(), labels, B, n, m->score_out);
        else score_labelled_rows(m, m->x.as<float>(), labels, B, n, m->score_out);
        if (m->score_labels_out) std::copy(labels, labels + (size_t)B * n, m->score_labels_out);
    }
    if (all_rows)   // each sequence's last row -> the loop's logits rows (what a decode step leaves there)
        HIPCHK(hipMemcpy2DAsync(m->logits.p, (size_t)V * 4, m->logits_all.as<float>() + (size_t)(n - 1) * V, (size_t)n * V * 4,
                                (size_t)V * 4, B, hipMemcpyDeviceToDevice, m->st));
    // the rows now stand at P + n; the greedy choice of their last logits feeds vc_decode_step(tok = NULL), as after a prefill
    std::vector<int> rec((size_t)B * RS_STRIDE);
    HIPCHK(hipMemcpyAsync(rec.data(), m->rows.p, rec.size() * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    for (int b = 0; b < B; ++b) rec[(size_t)b * RS_STRIDE + RS_POS] += n;
    HIPCHK(hipMemcpyAsync(m->rows.p, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, m->st));
    const LoopView v = session_view(m);
    enqueue_selection(m, v, v.logits, B, 0);
    m->cur_pos = P + n;
    m->tok_stale = false;
    if (logits_all)
        HIPCHK(hipMemcpyAsync(logits_all, m->logits_all.p, (size_t)B * n * V * 4, hipMemcpyDeviceToHost, m->st));
    if (logits_last) HIPCHK(hipMemcpyAsync(logits_last, m->logits.p, (size_t)B * V * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));   // `rec` is host memory
    GUARD_END(m->ctx)
}
