// engine_weights.inc — part of the host engine (textually included by engine.hip inside its anonymous namespace; one translation unit).
// device allocation helpers, HF key canonicalisation, the loader's 16-bit planes (hi / lo), place_tensor: every checkpoint tensor into its inference layout.

// the model that owns the weights and the model-wide settings (a session created by vc_model_create_shared points at its parent's)
template <class M> inline M* root_of(M* m) { return m->root ? m->root : m; }

template <class T> T* walloc(vc_model* m, size_t n, bool zero = false) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, rup(n * sizeof(T), 256)));
    if (zero) {
        HIPCHK(hipMemsetAsync(p, 0, rup(n * sizeof(T), 256), m->st));
        HIPCHK(hipStreamSynchronize(m->st));
    }
    m->owned.push_back(p);
    return reinterpret_cast<T*>(p);
}

void mark_needed(vc_model* m) {
    auto& n = m->need;
    const vc_model_cfg& c = m->c;
    n["model.embed_tokens.weight"] = false;
    n["lm_head.weight"] = false;
    n["model.norm.weight"] = false;
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".";
        for (const char* s : {"input_layernorm.weight", "post_attention_layernorm.weight", "self_attn.q_proj.weight",
                              "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                              "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight"})
            n[p + s] = false;
    }
    auto proj = [&](const std::string& prefix, int depth) {
        if (depth == 1) {
            n[prefix + ".weight"] = false;
            n[prefix + ".bias"] = false;
        }
        for (int j = 0; depth > 1 && j < depth; ++j) {
            n[prefix + "." + std::to_string(2 * j) + ".weight"] = false;
            n[prefix + "." + std::to_string(2 * j) + ".bias"] = false;
        }
    };
    proj("model.mm_projector", c.mm_proj_depth);
    if (c.variant != VC_VARIANT_LLAVA) proj("model.seg_mm_projector", c.seg_proj_depth);
    n["vit.embeddings.class_embedding"] = false;
    n["vit.embeddings.patch_embedding.weight"] = false;
    n["vit.embeddings.position_embedding.weight"] = false;
    n["vit.pre_layrnorm.weight"] = false;
    n["vit.pre_layrnorm.bias"] = false;
    for (int j = 0; j < c.vit_layers_used; ++j) {
        const std::string p = "vit.encoder.layers." + std::to_string(j) + ".";
        for (const char* s : {"layer_norm1", "layer_norm2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj",
                              "self_attn.out_proj", "mlp.fc1", "mlp.fc2"}) {
            n[p + s + ".weight"] = false;
            n[p + s + ".bias"] = false;
        }
    }
}

// canonical key: strips the CLIP prefixes of both Transformers generations (SURVEY.md Appendix A)
std::string canon_key(const std::string& k) {
    static const char* pre[] = {"model.vision_tower.vision_tower.vision_model.", "model.vision_tower.vision_tower.",
                                "vision_tower.vision_model.", "vision_model."};
    for (const char* p : pre) {
        const size_t n = strlen(p);
        if (k.compare(0, n, p) == 0) return "vit." + k.substr(n);
    }
    if (k.compare(0, 11, "embeddings.") == 0 || k.compare(0, 8, "encoder.") == 0 ||
        k.compare(0, 13, "pre_layrnorm.") == 0 || k.compare(0, 15, "post_layernorm.") == 0)
        return "vit." + k;
    return k;
}

// the lo plane of a weight (hi-plane pointer as loaded / packed), or nullptr: exact checkpoint, or none kept for it
const bf16_t* lo_plane(const vc_model* m, const void* hi) {
    const vc_model* r = root_of(m);
    auto it = r->lo_of.find(hi);
    return it == r->lo_of.end() ? nullptr : it->second;
}

// `n` elements of `src` -> elements [off, off + n) of the matrix at `base` (base_elems elements in all: q / k / v land in one
// matrix).  fp32 sources that bf16 cannot hold exactly get (and from then on fill) the matrix's lo plane.
void to_bf16(vc_model* m, bf16_t* base, size_t off, size_t base_elems, const void* src, int dtype, size_t n) {
    bf16_t* dst = base + off;
    auto it = m->lo_of.find(base);
    bf16_t* lo = it == m->lo_of.end() ? nullptr : it->second;
    if (dtype == VC_BF16) {
#if VC_OPERAND_FP16
        // the fp16-operand build: bfloat16 checkpoint bits are widened and take the fp32 path (fp16 holds every bf16 value of
        // magnitude 2^-17 .. 65504 exactly; what it cannot hold gets a lo plane like any other inexact tensor)
        m->cvt_tmp.ensure(n * 4);
        launch_truebf16_to_f32(reinterpret_cast<const uint16_t*>(src), m->cvt_tmp.as<float>(), n, m->st);
        src = m->cvt_tmp.p;
#else
        HIPCHK(hipMemcpyAsync(dst, src, n * 2, hipMemcpyDeviceToDevice, m->st));
        // a key loaded twice — an fp16 / fp32 source first (which made the lo plane), then a bf16 override (a projector-only
        // checkpoint saved in bf16): the exact reload must not leave the first load's lo values behind (ADVICE r5)
        if (lo) HIPCHK(hipMemsetAsync(lo + off, 0, n * 2, m->st));
        m->inexact_regions.erase({base, off});
        return;
#endif
    }
    if (!m->inexact_flag) m->inexact_flag = walloc<unsigned>(m, 64, true);
    HIPCHK(hipMemsetAsync(m->inexact_flag, 0, 4, m->st));
    launch_f32_to_bf16_planes(reinterpret_cast<const float*>(src), dst, lo ? lo + off : nullptr, n, m->inexact_flag, m->st);
    unsigned flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, m->inexact_flag, 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    if (!flag) {
        m->inexact_regions.erase({base, off});   // (an exact reload of a region: its lo values were just rewritten as zeros)
        return;
    }
    m->inexact_regions.insert({base, off});      // counted once per tensor, however often it is loaded
    if (!lo) {
        lo = walloc<bf16_t>(m, base_elems, true);   // zero: the parts of the matrix loaded from exact data
        m->lo_of[base] = lo;
        launch_f32_to_bf16_planes(reinterpret_cast<const float*>(src), dst, lo + off, n, nullptr, m->st);
    }
}
void to_bf16(vc_model* m, bf16_t* dst, const void* src, int dtype, size_t n) { to_bf16(m, dst, 0, n, src, dtype, n); }
void to_f32(vc_model* m, float* dst, const void* src, int dtype, size_t n) {
    if (dtype == VC_F32) HIPCHK(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, m->st));
    else launch_truebf16_to_f32(reinterpret_cast<const uint16_t*>(src), dst, n, m->st);   // checkpoint bits: bfloat16 in every build
}

// place a tensor that already sits on the device (`src`, dtype) into its inference layout
int place_tensor(vc_model* m, const std::string& raw_key, const void* src, int dtype, const int64_t* shape, int ndim) {
    const vc_model_cfg& c = m->c;
    const std::string key = canon_key(raw_key);
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    // full shape comparison (a transposed [K,N] matrix has the right element count and the wrong meaning); dimensions of
    // extent 1 are ignored so that [D] / [1,D] / [D,1,1] spellings of a vector all pass, and the patch embedding may come
    // as [Dv,3,P,P] or flattened [Dv, 3*P*P]
    auto expect = [&](std::initializer_list<int64_t> dims) {
        std::vector<int64_t> want, got;
        for (auto d : dims)
            if (d != 1) want.push_back(d);
        for (int i = 0; i < ndim; ++i)
            if (shape[i] != 1) got.push_back(shape[i]);
        bool ok = want == got;
        if (!ok && want.size() == 2 && got.size() > 2 && got[0] == want[0]) {  // conv weight [out, c, kh, kw]
            int64_t r = 1;
            for (size_t i = 1; i < got.size(); ++i) r *= got[i];
            ok = r == want[1];
        }
        if (!ok) {
            std::string w, g;
            for (auto d : want) w += (w.empty() ? "" : ",") + std::to_string(d);
            for (auto d : got) g += (g.empty() ? "" : ",") + std::to_string(d);
            REQUIRE(false, VC_ERR_INVALID, "%s: expected shape [%s], got [%s]", raw_key.c_str(), w.c_str(), g.c_str());
        }
    };
    const int D = c.hidden, F = c.ffn, V = c.vocab, Dv = c.vit_hidden, Fv = c.vit_ffn;
    // ---- dead at inference (SURVEY.md §0 quirks 1-3) or simply unused
    if (key.find("depth_mm_projector") != std::string::npos || key.find("mm2_projector") != std::string::npos ||
        key == "model.vcoder_lm_emb.weight" || key.compare(0, 19, "vit.post_layernorm.") == 0 ||
        key.find("position_ids") != std::string::npos || key.find("rotary_emb.inv_freq") != std::string::npos)
        return VC_IGNORED;
    if (c.variant == VC_VARIANT_LLAVA && key.find("seg_mm_projector") != std::string::npos) return VC_IGNORED;
    auto it = m->need.find(key);
    int layer = -1;
    char rest[128] = {0};
    if (sscanf(key.c_str(), "vit.encoder.layers.%d.%127s", &layer, rest) == 2 && layer >= c.vit_layers_used)
        return VC_IGNORED;  // layers after hidden_states[select_layer] are never evaluated
    REQUIRE(it != m->need.end(), VC_ERR_INVALID, "unexpected tensor key '%s'", raw_key.c_str());

    if (key == "model.embed_tokens.weight") { expect({V, D}); to_bf16(m, m->embed, src, dtype, numel); }
    else if (key == "lm_head.weight") { expect({V, D}); to_bf16(m, m->lm_head, src, dtype, numel); }
    else if (key == "model.norm.weight") { expect({D}); to_f32(m, m->final_norm, src, dtype, numel); }
    else if (sscanf(key.c_str(), "model.layers.%d.%127s", &layer, rest) == 2) {
        REQUIRE(layer >= 0 && layer < c.layers, VC_ERR_INVALID, "layer index out of range in %s", raw_key.c_str());
        LlmLayer& L = m->llm[layer];
        const std::string r = rest;
        if (r == "input_layernorm.weight") { expect({D}); to_f32(m, L.in_norm, src, dtype, numel); }
        else if (r == "post_attention_layernorm.weight") { expect({D}); to_f32(m, L.post_norm, src, dtype, numel); }
        else if (r == "self_attn.q_proj.weight") { expect({D, D}); to_bf16(m, L.qkv_w, 0, (size_t)3 * D * D, src, dtype, numel); }
        else if (r == "self_attn.k_proj.weight") { expect({D, D}); to_bf16(m, L.qkv_w, (size_t)D * D, (size_t)3 * D * D, src, dtype, numel); }
        else if (r == "self_attn.v_proj.weight") { expect({D, D}); to_bf16(m, L.qkv_w, (size_t)2 * D * D, (size_t)3 * D * D, src, dtype, numel); }
        else if (r == "self_attn.o_proj.weight") { expect({D, D}); to_bf16(m, L.o_w, src, dtype, numel); }
        else if (r == "mlp.gate_proj.weight") { expect({F, D}); to_bf16(m, L.gate_tmp, src, dtype, numel); }
        else if (r == "mlp.up_proj.weight") { expect({F, D}); to_bf16(m, L.up_tmp, src, dtype, numel); }
        else if (r == "mlp.down_proj.weight") { expect({D, F}); to_bf16(m, L.down_w, src, dtype, numel); }
        else REQUIRE(false, VC_ERR_INVALID, "unexpected tensor key '%s'", raw_key.c_str());
    } else if (key.compare(0, 19, "model.mm_projector.") == 0 || key.compare(0, 23, "model.seg_mm_projector.") == 0) {
        const bool is_seg = key.compare(0, 23, "model.seg_mm_projector.") == 0;
        Projector& pj = is_seg ? m->seg : m->mm;
        const std::string r = key.substr(is_seg ? 23 : 19);
        int idx = 0;
        char what[32] = {0};
        if (sscanf(r.c_str(), "%d.%31s", &idx, what) == 2) idx /= 2;
        else { idx = 0; snprintf(what, sizeof what, "%s", r.c_str()); }
        REQUIRE(idx >= 0 && idx < pj.depth, VC_ERR_INVALID, "projector layer out of range in %s", raw_key.c_str());
        const int in = idx == 0 ? Dv : D;
        if (!strcmp(what, "weight")) { expect({D, in}); to_bf16(m, pj.w[idx], src, dtype, numel); }
        else { expect({D}); to_f32(m, pj.b[idx], src, dtype, numel); }
    } else if (key == "vit.embeddings.class_embedding") { expect({Dv}); to_f32(m, m->vit_cls, src, dtype, numel); }
    else if (key == "vit.embeddings.position_embedding.weight") { expect({m->Tv, Dv}); to_f32(m, m->vit_pos, src, dtype, numel); }
    else if (key == "vit.embeddings.patch_embedding.weight") {
        expect({Dv, m->Kpatch});
        m->stage2.ensure(numel * 2);
        m->lo_of.erase(m->stage2.p);
        to_bf16(m, m->stage2.as<bf16_t>(), src, dtype, numel);
        HIPCHK(hipMemcpy2DAsync(m->vit_patch_w, (size_t)m->Kpad * 2, m->stage2.p, (size_t)m->Kpatch * 2,
                                (size_t)m->Kpatch * 2, Dv, hipMemcpyDeviceToDevice, m->st));
        if (auto it2 = m->lo_of.find(m->stage2.p); it2 != m->lo_of.end()) {   // the staged lo plane -> the padded [Dv, Kpad] layout
            bf16_t* lo_pad = walloc<bf16_t>(m, (size_t)Dv * m->Kpad, true);
            HIPCHK(hipMemcpy2DAsync(lo_pad, (size_t)m->Kpad * 2, it2->second, (size_t)m->Kpatch * 2, (size_t)m->Kpatch * 2, Dv,
                                    hipMemcpyDeviceToDevice, m->st));
            m->lo_of.erase(it2);
            m->lo_of[m->vit_patch_w] = lo_pad;
        }
    } else if (key == "vit.pre_layrnorm.weight") { expect({Dv}); to_f32(m, m->vit_pre_w, src, dtype, numel); }
    else if (key == "vit.pre_layrnorm.bias") { expect({Dv}); to_f32(m, m->vit_pre_b, src, dtype, numel); }
    else if (sscanf(key.c_str(), "vit.encoder.layers.%d.%127s", &layer, rest) == 2) {
        VitLayer& L = m->vit[layer];
        const std::string r = rest;
        const size_t DD = (size_t)Dv * Dv;
        if (r == "layer_norm1.weight") { expect({Dv}); to_f32(m, L.ln1_w, src, dtype, numel); }
        else if (r == "layer_norm1.bias") { expect({Dv}); to_f32(m, L.ln1_b, src, dtype, numel); }
        else if (r == "layer_norm2.weight") { expect({Dv}); to_f32(m, L.ln2_w, src, dtype, numel); }
        else if (r == "layer_norm2.bias") { expect({Dv}); to_f32(m, L.ln2_b, src, dtype, numel); }
        else if (r == "self_attn.q_proj.weight") { expect({Dv, Dv}); to_bf16(m, L.qkv_w, 0, 3 * DD, src, dtype, numel); }
        else if (r == "self_attn.k_proj.weight") { expect({Dv, Dv}); to_bf16(m, L.qkv_w, DD, 3 * DD, src, dtype, numel); }
        else if (r == "self_attn.v_proj.weight") { expect({Dv, Dv}); to_bf16(m, L.qkv_w, 2 * DD, 3 * DD, src, dtype, numel); }
        else if (r == "self_attn.q_proj.bias") { expect({Dv}); to_f32(m, L.qkv_b, src, dtype, numel); }
        else if (r == "self_attn.k_proj.bias") { expect({Dv}); to_f32(m, L.qkv_b + Dv, src, dtype, numel); }
        else if (r == "self_attn.v_proj.bias") { expect({Dv}); to_f32(m, L.qkv_b + 2 * Dv, src, dtype, numel); }
        else if (r == "self_attn.out_proj.weight") { expect({Dv, Dv}); to_bf16(m, L.out_w, src, dtype, numel); }
        else if (r == "self_attn.out_proj.bias") { expect({Dv}); to_f32(m, L.out_b, src, dtype, numel); }
        else if (r == "mlp.fc1.weight") { expect({Fv, Dv}); to_bf16(m, L.fc1_w, src, dtype, numel); }
        else if (r == "mlp.fc1.bias") { expect({Fv}); to_f32(m, L.fc1_b, src, dtype, numel); }
        else if (r == "mlp.fc2.weight") { expect({Dv, Fv}); to_bf16(m, L.fc2_w, src, dtype, numel); }
        else if (r == "mlp.fc2.bias") { expect({Dv}); to_f32(m, L.fc2_b, src, dtype, numel); }
        else REQUIRE(false, VC_ERR_INVALID, "unexpected tensor key '%s'", raw_key.c_str());
    } else {
        REQUIRE(false, VC_ERR_INVALID, "unexpected tensor key '%s'", raw_key.c_str());
    }
    it->second = true;
    HIPCHK(hipStreamSynchronize(m->st));  // staging buffers are reused by the next call
    return VC_OK;
}

// the session's key mask (keys hidden by the caller's attention_mask: [VC_MAX_ROWS][max_positions] bytes, 0 = hidden) onto the
// arguments of an attention launch, when `on` (a prefill: m->has_kmask; cached rows: m->kmask_in_decode)
template <class A> void attach_kmask(const vc_model* m, A& a, bool on) {
    if (!on) return;
    a.key_mask = m->kmask.as<uint8_t>();
    a.mask_stride = m->c.max_positions;
}

// output_hidden_states hook (defined with the prefill layers); x_src: the residual rows to copy (default: the prefill's m->x)
void emit_hidden(vc_model* m, int idx, int B, int S, const float* x_src = nullptr);
// output_attentions hook: the probabilities of decoder layer l from its q / k in the precision mode's own form.  S queries
// starting at position q_pos0 against Tk keys (0: S — a prefill; a cached decode step: S = 1, Tk = its position + 1)
void emit_attentions(vc_model* m, int l, int B, int S, AttnProbsArgs a, int Tk = 0, int q_pos0 = 0) {
    if (!m->attn_out) return;
    const int keys = Tk > 0 ? Tk : S;
    const size_t n = (size_t)B * m->c.heads * S * keys;
    REQUIRE((size_t)(l + 1) * n <= m->attn_cap, VC_ERR_INVALID, "attention buffer too small: %zu floats for layer %d of %zu", m->attn_cap,
            l, n);
    REQUIRE(keys <= 4096, VC_ERR_INVALID, "output_attentions: at most 4096 positions");
    m->hidden_tmp.ensure(n * 4);
    a.out = m->hidden_tmp.as<float>();
    a.B = B;
    a.H = m->c.heads;
    a.T = S;
    a.Tk = Tk;
    a.q_pos0 = q_pos0;
    a.hd = m->hd;
    a.scale = 1.0f / sqrtf((float)m->hd);
    attach_kmask(m, a, Tk > 0 ? m->kmask_in_decode : m->has_kmask);
    launch_attn_probs(a, m->st);
    HIPCHK(hipMemcpyAsync(m->attn_out + (size_t)l * n, a.out, n * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));   // hidden_tmp is shared with the hidden-state hook
}

