// engine_llm.inc — part of the host engine (textually included by engine.hip inside its anonymous namespace; one translation unit).
// splice planner, prefill workspaces and KV caches, the decoder stack of a prefill (bf16 / fp8 / split / strict), the decode step and its hipGraph, RowState records, select arguments.

// ------------------------------------------------------------------------------------------------
// splice planner (host).  One (kind, src) pair per destination row of inputs_embeds.
struct RowSrc { int kind, src; };

// `labels` [B, T] (nullptr: none announced): lab_out[b] receives one label per destination row, by the plan the embeddings follow
// — a text row carries the label of its id, a feature row IGNORE_INDEX, text the DS variant drops between <image> and <seg> drops
// its label with it, and whatever stands at a placeholder position of `labels` is never read (vcoder_ds_llava_arch.py:176, 203-204,
// 213-216, 225-228, 239-241, 254-257, 269-270; a row without placeholders passes its labels through, :181-208).
void plan_rows(vc_model* m, const int64_t* ids, int B, int T, bool has_seg, const std::vector<bool>* depth_zero,
               int R, std::vector<std::vector<RowSrc>>& out, const int64_t* labels = nullptr,
               std::vector<std::vector<int64_t>>* lab_out = nullptr) {
    const int variant = m->c.variant;
    int img_i = 0, seg_i = 0, dep_i = 0;
    std::vector<int64_t>* lab = nullptr;   // the labels of the row being planned
    auto text = [&](std::vector<RowSrc>& rows, const int64_t* p, int n) {
        for (int i = 0; i < n; ++i) {
            REQUIRE(p[i] >= 0 && p[i] < m->c.vocab, VC_ERR_INDEX,
                    "index out of range in self (id %lld reached the embedding lookup)", (long long)p[i]);
            rows.push_back({0, (int)p[i]});
            if (lab) lab->push_back(labels[(p - ids) + i]);
        }
    };
    // features[idx] of the reference: the block of sample idx — R rows per image, all images of the sample flattened
    // (`[x.flatten(0, 1) for x in image_features]`, vcoder_ds_llava_arch.py:143); one image per sample in the 4-D form
    auto feat = [&](std::vector<RowSrc>& rows, int mod, int idx, bool emit) {
        const std::vector<int>& first = m->img_first[mod];
        const int nblocks = first.empty() ? m->feat_rows[mod] / R : (int)first.size() - 1;
        REQUIRE(idx < nblocks, VC_ERR_INDEX, "index %d is out of bounds for dimension 0 with size %d", idx, nblocks);
        const int i0 = first.empty() ? idx : first[idx], i1 = first.empty() ? idx + 1 : first[idx + 1];
        for (int r = i0 * R; emit && r < i1 * R; ++r) {
            rows.push_back({1, m->feat_off[mod] + r});
            if (lab) lab->push_back(IGNORE_INDEX);
        }
    };
    auto find = [](const int64_t* p, int n, int tok) {
        for (int i = 0; i < n; ++i)
            if (p[i] == tok) return i;
        return -1;
    };
    out.assign(B, {});
    if (labels && lab_out) lab_out->assign(B, {});
    for (int b = 0; b < B; ++b) {
        const int64_t* cur = ids + (size_t)b * T;
        int n = T;
        std::vector<RowSrc>& rows = out[b];
        lab = labels && lab_out ? &(*lab_out)[b] : nullptr;
        int n_img = 0, n_seg = 0;
        for (int i = 0; i < T; ++i) {
            n_img += cur[i] == IMAGE_TOKEN_INDEX;
            n_seg += cur[i] == SEG_TOKEN_INDEX;
        }
        // "not multimodal" guard: llava_arch.py:118, vcoder_llava_arch.py:187 (`or`), vcoder_ds_llava_arch.py:181 (`and`)
        const bool plain = variant == VC_VARIANT_LLAVA ? n_img == 0
                           : variant == VC_VARIANT_VCODER ? (n_img == 0 || n_seg == 0)
                                                          : (n_img == 0 && n_seg == 0);
        if (plain) {
            feat(rows, VC_MOD_IMAGE, img_i, false);  // the reference indexes the features before embedding the ids
            if (variant != VC_VARIANT_LLAVA && has_seg) feat(rows, VC_MOD_SEG, seg_i, false);
            text(rows, cur, n);
            ++img_i; ++seg_i; ++dep_i;
            continue;
        }
        for (int at; (at = find(cur, n, IMAGE_TOKEN_INDEX)) >= 0;) {
            feat(rows, VC_MOD_IMAGE, img_i, false);
            text(rows, cur, at);
            feat(rows, VC_MOD_IMAGE, img_i++, true);
            cur += at + 1;
            n -= at + 1;
        }
        if (variant != VC_VARIANT_LLAVA && has_seg) {
            for (int at; (at = find(cur, n, SEG_TOKEN_INDEX)) >= 0;) {
                feat(rows, VC_MOD_SEG, seg_i, false);
                if (variant == VC_VARIANT_VCODER) text(rows, cur, at);  // vcoder_llava_arch.py:236 keeps the text,
                feat(rows, VC_MOD_SEG, seg_i++, true);                  // vcoder_ds_llava_arch.py:238 drops it
                cur += at + 1;
                n -= at + 1;
            }
        }
        if (variant == VC_VARIANT_VCODER_DS) {
            // a row with several <depth> placeholders advances the depth index more than once: later rows then index past
            // the per-sample list, where the reference raises IndexError (vcoder_ds_llava_arch.py:246)
            REQUIRE(!depth_zero || dep_i < (int)depth_zero->size(), VC_ERR_INDEX, "list index out of range (depth index %d of %zu)",
                    dep_i, depth_zero ? depth_zero->size() : (size_t)0);
            const bool dz = depth_zero ? (*depth_zero)[dep_i] : true;
            if (!dz) {
                for (int at; (at = find(cur, n, DEPTH_TOKEN_INDEX)) >= 0;) {
                    feat(rows, VC_MOD_DEPTH, dep_i, false);
                    text(rows, cur, at);
                    feat(rows, VC_MOD_DEPTH, dep_i++, true);
                    cur += at + 1;
                    n -= at + 1;
                }
            } else {
                ++dep_i;
            }
        }
        if (n > 0) text(rows, cur, n);
    }
}

// workspaces of a prefill of B sequences of up to Scap rows (independent of where the KV cache lives)
void ensure_prefill_ws(vc_model* m, int B, int Scap) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn;
    const size_t Mrows = (size_t)B * Scap;
    m->x.ensure(Mrows * D * 4);
    m->xn.ensure(Mrows * (D + XN_PAD) * 2);
    m->qkv.ensure(Mrows * 3 * D * 2);
    m->q.ensure(Mrows * D * 2, true);
    m->attn.ensure(Mrows * D * 2);
    m->h.ensure(Mrows * F * 2);
    if (m->weight_format == 2) {
        m->a8.ensure(Mrows * std::max(D, F));
        m->a8_scale.ensure(Mrows * 4);
    }
    m->row_src.ensure(Mrows * 8);
    m->p_ssq.ensure(Mrows * (size_t)m->npart * 4);   // folded RMSNorm of the prefill: sum-of-squares partials + row scales
    m->p_rstd.ensure(Mrows * 4);
    const int Bp = (int)rup(B, 16);
    m->last_idx.ensure(Bp * 4);
    m->xl.ensure((size_t)Bp * D * 2, true);
    m->logits.ensure((size_t)Bp * c.vocab * 4, true);
}

// every captured step of the session goes: for what a step bakes in without it showing in its StepKey (see there)
void drop_graph(vc_model* m) {
    for (StepGraph& s : m->step)
        if (s.exec) {
            (void)hipGraphExecDestroy(s.exec);
            s.exec = nullptr;
        }
}

// the session's own decode loop: KV cache for B sequences of S_total positions + the per-step buffers
void ensure_llm(vc_model* m, int B, int S_total) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn, H = c.heads;
    const int Scap = (int)rup(S_total, 64);
    REQUIRE(B <= VC_MAX_ROWS, VC_ERR_INVALID, "batch %d: at most %d sequences per GPU replica (shard larger batches over ranks)",
            B, VC_MAX_ROWS);
    REQUIRE(Scap <= c.max_positions, VC_ERR_INVALID, "sequence %d exceeds max_position_embeddings=%d", Scap, c.max_positions);
    // split mode keeps fp24 (or fp32) keys / values; the fp8 weight format e4m3 ones
    const int es = m->precision == 2 ? split_kv_es() : (m->precision == 0 ? step_kv_es(m) : 2);
    if (B != m->capB || Scap > m->capS || es != m->kv_es) {
        const int newS = std::max(Scap, (m->capB == B && es == m->kv_es) ? m->capS : 0);
        const size_t per_layer = (size_t)B * H * newS * m->hd;
        m->kc.release();
        m->vc.release();
        m->kc.ensure(per_layer * c.layers * es, true);
        m->vc.ensure(per_layer * c.layers * es, true);
        m->capB = B;
        m->capS = newS;
        m->kv_es = es;
    }
    ensure_prefill_ws(m, B, Scap);
    const int Bp = (int)rup(B, 16);
    // (sized for the split step as well: hi + lo row groups double the bf16 operands, qkv_dec is fp32 there)
    m->x_dec.ensure((size_t)Bp * D * 4, true);
    m->xg_dec.ensure((size_t)2 * Bp * D * 2, true);
    m->qkv_dec.ensure((size_t)Bp * 3 * D * 4, true);
    m->attn_dec.ensure((size_t)2 * Bp * D * 2, true);
    m->h_dec.ensure((size_t)2 * Bp * F * 2, true);
    m->next_tok.ensure(Bp * 4, true);
    m->rows.ensure((size_t)Bp * RS_STRIDE * 4, true);
    m->ssq.ensure((size_t)Bp * m->npart * 4, true);
    m->sk_scratch.ensure(sk_floats(c) * 4);   // [K-slices][tiles][2 row groups][256]
    m->sk_counters.ensure((size_t)sk_counters_n(c) * 4, true);
}

// the plain step of the session's loop: no log-prob slabs, no processor buffers (a generate() call attaches its own to a copy)
LoopView session_view(vc_model* m) {
    LoopView v{};
    v.st = m->st;
    v.kc = m->kc.as<bf16_t>();
    v.vc = m->vc.as<bf16_t>();
    v.es = m->kv_es;
    v.split_G = m->precision == 2 ? (m->capB <= 8 ? 8 : 16) : 0;
    v.capR = m->capB;
    v.capS = m->capS;
    v.rows = m->rows.as<int>();
    v.kmask = m->kmask_in_decode ? m->kmask.as<uint8_t>() : nullptr;
    v.kmask_stride = m->c.max_positions;
    v.x_dec = m->x_dec.as<float>();
    v.xg_dec = m->xg_dec.as<bf16_t>();
    v.qkv_dec = m->qkv_dec.as<bf16_t>();
    v.attn_dec = m->attn_dec.as<bf16_t>();
    v.h_dec = m->h_dec.as<bf16_t>();
    v.logits = m->logits.as<float>();
    v.next_tok = m->next_tok.as<int>();
    v.out_ids = m->out_ids.as<int>();
    v.ssq = m->ssq.as<float>();
    v.sk_scratch = m->sk_scratch.as<float>();
    v.sk_counters = m->sk_counters.as<unsigned>();
    return v;
}

// where a prefill writes its keys / values: rows [row0, row0 + B) of a cache with capR rows of capS positions
struct KvTarget {
    bf16_t *kc, *vc;
    int capR, capS, row0;
    int es;  // bytes per element: 2 (bf16); precision mode "split": 3 (fp24) or 4 (fp32)
};
// row t.row0 of layer l of a cache whose elements are t.es bytes (the pointer type is nominal for es != 2)
bf16_t* kv_layer(const vc_model* m, bf16_t* base, const KvTarget& t, int l) {
    const size_t elems = ((size_t)l * t.capR + t.row0) * m->c.heads * t.capS * m->hd;
    return reinterpret_cast<bf16_t*>(reinterpret_cast<char*>(base) + elems * t.es);
}
bf16_t* kcache(const vc_model* m, const KvTarget& t, int l) { return kv_layer(m, t.kc, t, l); }
bf16_t* vcache(const vc_model* m, const KvTarget& t, int l) { return kv_layer(m, t.vc, t, l); }
KvTarget session_kv(vc_model* m) { return KvTarget{m->kc.as<bf16_t>(), m->vc.as<bf16_t>(), m->capB, m->capS, 0, m->kv_es}; }
KvTarget loop_kv(const LoopView& v) { return KvTarget{v.kc, v.vc, v.capR, v.capS, 0, v.es}; }   // all rows of a loop's cache

// The decode loop outran the cache (a host-driven vc_decode_step loop past the reserve of its prefill): re-allocate with
// room for `need` positions and move the live prefix — K and V rows are contiguous per (layer, sample, head), so each is
// one strided 2-D copy.  (The captured steps are keyed on the cache pointers and capS: the next one is re-captured.)
void grow_kv(vc_model* m, int need) {
    const vc_model_cfg& c = m->c;
    const int oldS = m->capS, live = m->cur_pos;
    int newS = (int)rup(std::max(need, std::min(2 * oldS, c.max_positions)), 64);
    newS = std::min(newS, c.max_positions / 64 * 64);
    REQUIRE(newS >= need, VC_ERR_STATE, "KV cache full: position %d exceeds max_position_embeddings=%d", need, c.max_positions);
    const size_t heads = (size_t)c.layers * m->capB * c.heads;
    Buf nk, nv;
    const size_t es = (size_t)m->kv_es;
    nk.ensure(heads * newS * m->hd * es, true);
    nv.ensure(heads * newS * m->hd * es, true);
    HIPCHK(hipMemcpy2DAsync(nk.p, (size_t)newS * m->hd * es, m->kc.p, (size_t)oldS * m->hd * es, (size_t)live * m->hd * es, heads,
                            hipMemcpyDeviceToDevice, m->st));
    HIPCHK(hipMemcpy2DAsync(nv.p, (size_t)newS * m->hd * es, m->vc.p, (size_t)oldS * m->hd * es, (size_t)live * m->hd * es, heads,
                            hipMemcpyDeviceToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    m->kc.release();
    m->vc.release();
    m->kc = nk;
    m->vc = nv;
    if (m->precision == 1 && m->s_capS == oldS && m->s_capB == m->capB) {  // the strict path's fp32 caches (K and V key-major)
        Buf sk, sv;
        sk.ensure(heads * newS * m->hd * 4, true);
        sv.ensure(heads * newS * m->hd * 4, true);
        HIPCHK(hipMemcpy2DAsync(sk.p, (size_t)newS * m->hd * 4, m->s_kc.p, (size_t)oldS * m->hd * 4, (size_t)live * m->hd * 4,
                                heads, hipMemcpyDeviceToDevice, m->st));
        HIPCHK(hipMemcpy2DAsync(sv.p, (size_t)newS * m->hd * 4, m->s_vc.p, (size_t)oldS * m->hd * 4, (size_t)live * m->hd * 4,
                                heads, hipMemcpyDeviceToDevice, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        m->s_kc.release();
        m->s_vc.release();
        m->s_kc = sk;
        m->s_vc = sv;
        m->s_capS = newS;
    }
    m->capS = newS;
}

// output_hidden_states ([HF] LlamaModel.forward: the tuple (inputs_embeds, layer 1 output, ..., layer L-1 output,
// norm(layer L output))): entry `idx` of the caller's host buffer <- the fp32 residual stream (idx == layers: after the final
// RMSNorm).  No-op unless requested for this prefill.
void emit_hidden(vc_model* m, int idx, int B, int S, const float* x_src) {
    if (!m->hidden_out) return;
    const vc_model_cfg& c = m->c;
    const size_t n = (size_t)B * S * c.hidden;
    REQUIRE((size_t)(idx + 1) * n <= m->hidden_cap, VC_ERR_INVALID, "hidden-state buffer too small: %zu floats for entry %d of %zu",
            m->hidden_cap, idx, n);
    const float* src = x_src ? x_src : m->x.as<float>();
    if (idx == c.layers) {
        m->hidden_tmp.ensure(n * 4);
        launch_rmsnorm_f32(src, nullptr, m->final_norm, m->hidden_tmp.as<float>(), B * S, c.hidden, c.rms_eps, m->st);
        src = m->hidden_tmp.as<float>();
    }
    HIPCHK(hipMemcpyAsync(m->hidden_out + (size_t)idx * n, src, n * 4, hipMemcpyDeviceToHost, m->st));
}

// ---- the linears of a decoder layer around its attention, stated once for the prefill and vc_extend ------------------------------
// Folded RMSNorm of a prefill (VC_PREFILL_FOLD, see run_prefill_layers): the arguments of the GEMMs that produce xg / consume
// 1/rms, and whether xn already holds bf16(x * g) of the CURRENT x for the norm about to be consumed (rstd: its row scales)
struct FoldRun {
    bool on = false;
    NormFold prod, cons;
    bool have_xg = false;
};
FoldRun fold_run(vc_model* m, bool on, int ld_xg, int xg_lo) {
    FoldRun fr;
    fr.on = on;
    fr.prod = NormFold{nullptr, m->xn.as<bf16_t>(), nullptr, m->p_ssq.as<float>(), ld_xg, xg_lo, m->npart};
    fr.cons = NormFold{m->p_rstd.as<float>()};
    return fr;
}
// the unfused QKV projection of precision mode 0 over the M rows of m->x: RMSNorm -> GEMM into m->qkv [M, 3D] (fp8 format: the
// norm writes the e4m3 operand of the GEMM directly).  With `qe` the GEMM runs the fused epilogue instead (EPI_QKV: no [M, 3D]
// rows; its token rows are the samples padded to Tp).
void qkv_projection(vc_model* m, const LlmLayer& L, int M, const FoldRun& fr, const QkvEpiArgs* qe = nullptr) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, Mg = qe ? qe->B * qe->Tp : M, ldo = qe ? 0 : 3 * D, epi = qe ? EPI_QKV : EPI_BF16;
    void* out = qe ? nullptr : m->qkv.p;
    if (m->weight_format == 2) {
        launch_rmsnorm_q8(m->x.as<float>(), L.in_norm, m->a8.as<uint8_t>(), m->a8_scale.as<float>(), M, D, c.rms_eps, m->st);
        gemm_f8(m, nullptr, L.qkv_q, L.qkv_s, out, Mg, 3 * D, D, ldo, epi, qe);
    } else {
        if (!fr.have_xg) launch_rmsnorm(m->x.as<float>(), L.in_norm, m->xn.as<bf16_t>(), M, D, c.rms_eps, m->st, D + XN_PAD);
        gemm(m, m->xn.as<bf16_t>(), L.qkv_w, nullptr, out, Mg, 3 * D, D, ldo, epi, D + XN_PAD, fr.have_xg ? &fr.cons : nullptr, qe);
    }
}
// The tail of a decoder layer behind its attention: o_proj (+ residual) -> post norm -> gate / up (SwiGLU) -> down (+ residual)
// over the M rows of m->x, on bf16-valued operands m->attn / m->xn / m->h with row strides ld_attn / ld_xn / ld_h.
//   mm(A, lda, W, out, N, K, ldo, epi, lo_off, fold): the mode's GEMM wrapper (lo_off: gemm_split's split_out)
//   norm(w): the mode's RMSNorm pass m->x -> m->xn
// Folded (fr.on): no norm pass — o_proj and down also write xg for the next GEMM and the rows' sum-of-squares partials, a
// one-wave-per-row launch turns them into 1/rms; next_in: the norm the layer's output meets next (nullptr: the last layer's
// output meets the final norm on its gathered rows only).
struct TailLd { int attn, xn, h, h_lo; };
template <class Gemm, class Norm>
void layer_tail_on(vc_model* m, const LlmLayer& L, int M, const TailLd& ld, Gemm&& mm, Norm&& norm, FoldRun& fr, const float* next_in) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn;
    NormFold* prod = fr.on ? &fr.prod : nullptr;
    auto rstd = [&] { launch_rstd_from_partials(prod->ssq_out, m->npart, D / 16, m->p_rstd.as<float>(), M, D, c.rms_eps, m->st); };
    if (prod) prod->xg_w = L.post_norm;
    mm(m->attn.as<bf16_t>(), ld.attn, L.o_w, m->x.p, D, D, D, EPI_RESID_F32, 0, prod);
    if (prod) rstd();
    else norm(L.post_norm);
    mm(m->xn.as<bf16_t>(), ld.xn, L.gu_w, m->h.p, 2 * F, D, ld.h, EPI_SWIGLU, ld.h_lo, prod ? &fr.cons : nullptr);
    fr.have_xg = prod && next_in;
    if (prod) prod->xg_w = next_in;
    mm(m->h.as<bf16_t>(), ld.h, L.down_w, m->x.p, D, F, D, EPI_RESID_F32, 0, fr.have_xg ? prod : nullptr);
    if (fr.have_xg) rstd();
}
// ... of precision mode 0: bf16 weights, or the fp8 format's W8A8 GEMMs (never folded)
void layer_tail(vc_model* m, const LlmLayer& L, int M, FoldRun& fr, const float* next_in) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn;
    if (m->weight_format == 2) {
        gemm_f8(m, m->attn.as<bf16_t>(), L.o_q, L.o_s, m->x.p, M, D, D, D, EPI_RESID_F32);
        launch_rmsnorm_q8(m->x.as<float>(), L.post_norm, m->a8.as<uint8_t>(), m->a8_scale.as<float>(), M, D, c.rms_eps, m->st);
        gemm_f8(m, nullptr, L.gu_q, L.gu_s, m->h.p, M, 2 * F, D, F, EPI_SWIGLU);
        gemm_f8(m, m->h.as<bf16_t>(), L.down_q, L.down_s, m->x.p, M, D, F, D, EPI_RESID_F32);
        return;
    }
    layer_tail_on(
        m, L, M, TailLd{D, D + XN_PAD, F, 0},
        [&](const bf16_t* A, int lda, const bf16_t* W, void* out, int N, int K, int ldo, int epi, int, const NormFold* fold) {
            gemm(m, A, W, nullptr, out, M, N, K, ldo, epi, lda, fold);
        },
        [&](const float* w) { launch_rmsnorm(m->x.as<float>(), w, m->xn.as<bf16_t>(), M, D, c.rms_eps, m->st, D + XN_PAD); }, fr, next_in);
}

// decoder layers [l0, l1) of a prefill (l1 < 0: all, or the first layer_limit)
void run_prefill_layers(vc_model* m, const KvTarget& kv, int B, int S, int l0 = 0, int l1 = -1) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, H = c.heads, M = B * S;
    const int nl = l1 >= 0 ? l1 : (m->layer_limit > 0 ? std::min(m->layer_limit, c.layers) : c.layers);
    const int Sr = (int)rup(S, 64);
    m->vt_pre.ensure((size_t)B * H * m->hd * Sr * 2, true);
    if (kv.es == 1) m->k_pre.ensure((size_t)B * H * Sr * m->hd * 2, true);
    const bool f8 = m->weight_format == 2;
    // VC_PREFILL_FOLD=1 (opt-in; read per call so that tests can switch it): RMSNorm never runs as a pass behind the first
    // layer — the GEMM that writes a residual row (o_proj, down) also writes xg = bf16(x * g) for the next GEMM and the row's
    // sum-of-squares partials, a one-wave-per-row launch turns them into 1/rms, and the consuming GEMM (gate/up, the next
    // layer's QKV) scales its accumulator by it: the decode steps' form (DESIGN.md section 2).  Measured on MI355X (7b, B = 8,
    // profiles/r04_d_*): 112.9 ms per prefill against 111.6 with the 63 passes — the residual GEMMs' epilogue (8-byte bf16
    // stores in 32-byte segments, partials) costs more than the 45-us passes it removes — so the passes stay the default.
    FoldRun fr = fold_run(m, prefill_fold_on() && !f8, D + XN_PAD, 0);
    // the fused QKV epilogue: hd 128, two heads per 256-row weight tile, a problem the 256 x 256 kernel serves anyway
    const int qf = root_of(m)->qkv_fused;
    const bool qkv_fused = qf && m->hd == 128 && D % 256 == 0 && (qf > 1 || (long)B * rup(S, 32) >= 1024);
    for (int l = l0; l < nl; ++l) {
        const LlmLayer& L = m->llm[l];
        // K and V rows go to the cache (key-major: what the decode steps stream); the V^T tiles of this layer's flash
        // attention live in a per-call scratch [B,H,hd,Sr]
        // (kv.es == 1, the e4m3 cache of the fp8 format: the flash kernel of THIS prefill reads bf16 K rows from a per-call
        // scratch, the cache receives e4m3 rows)
        const bool kv8 = kv.es == 1;
        bf16_t* kflash = kv8 ? m->k_pre.as<bf16_t>() : kcache(m, kv, l);
        const int kflash_stride = kv8 ? Sr : kv.capS;
        // round 6 (SURVEY K13): RoPE + head split + KV write in the QKV GEMM's epilogue — the fused [M, 3D] rows are never
        // written and qkv_split_kernel's pass (105 us per 7b layer at B = 8, 263 us at 13b B = 16) is gone.  The token rows of that
        // GEMM are the samples padded to a multiple of 32 (EPI_QKV, kernels.h); same bits as the two launches it replaces.
        const int Sp = (int)rup(S, 32);
        if (qkv_fused) {
            QkvEpiArgs qe{m->q.as<bf16_t>(), kflash, kv8 ? nullptr : vcache(m, kv, l), m->vt_pre.as<bf16_t>(),
                          kv8 ? reinterpret_cast<uint8_t*>(kcache(m, kv, l)) : nullptr,
                          kv8 ? reinterpret_cast<uint8_t*>(vcache(m, kv, l)) : nullptr, m->rope_cos, m->rope_sin, B, S, Sp, H, S,
                          kflash_stride, Sr, kv.capS};
            qkv_projection(m, L, M, fr, &qe);
        } else {
            qkv_projection(m, L, M, fr);
            QkvSplitArgs qa{m->qkv.as<bf16_t>(), m->q.as<bf16_t>(), kflash, m->vt_pre.as<bf16_t>(), B, S, H, m->hd, S, kflash_stride,
                            nullptr, m->rope_cos, m->rope_sin, kv8 ? nullptr : vcache(m, kv, l), Sr,
                            kv8 ? reinterpret_cast<uint8_t*>(kcache(m, kv, l)) : nullptr,
                            kv8 ? reinterpret_cast<uint8_t*>(vcache(m, kv, l)) : nullptr, kv.capS};
            launch_qkv_split(qa, m->st);
        }
        AttnArgs aa{m->q.as<bf16_t>(), kflash, m->vt_pre.as<bf16_t>(), m->attn.as<bf16_t>(), B, H, S, m->hd, S, kflash_stride, 1,
                    1.0f / sqrtf((float)m->hd), Sr};
        attach_kmask(m, aa, m->has_kmask);
        launch_attention(aa, m->st);
        if (m->attn_out) {
            AttnProbsArgs pa{};
            pa.q_hi = m->q.as<bf16_t>();
            pa.k_hi = kflash;
            pa.q_stride = S;
            pa.kv_stride = kflash_stride;
            emit_attentions(m, l, B, S, pa);
        }
        layer_tail(m, L, M, fr, l + 1 < nl ? m->llm[l + 1].in_norm : nullptr);
        emit_hidden(m, l + 1, B, S);
    }
}

// the decoder stack of a prefill in precision mode "split": fp32 keys / values go to `kv` (es == 4), the bf16 hi / lo
// planes the flash kernel needs live in per-call scratch
void run_prefill_layers_split(vc_model* m, const KvTarget& kv, int B, int S, int l0 = 0, int l1 = -1) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn, H = c.heads, M = B * S;
    const int nl = l1 >= 0 ? l1 : (m->layer_limit > 0 ? std::min(m->layer_limit, c.layers) : c.layers);
    const int Sr = (int)rup(S, 64);
    const int ldx = split_ld(D), ldh = split_ld(F);
    REQUIRE(kv.es == 3 || kv.es == 4, VC_ERR_STATE, "split mode needs an fp24 / fp32 KV cache");
    const size_t qplane = (size_t)B * H * S * m->hd, kplane = (size_t)B * H * Sr * m->hd;
    m->xn.ensure((size_t)M * ldx * 2);
    m->s_qkv.ensure((size_t)M * 3 * D * 4);
    m->q.ensure(2 * qplane * 2, true);
    m->vt_pre.ensure(4 * kplane * 2, true);   // K hi | K lo | V^T hi | V^T lo
    m->attn.ensure((size_t)M * ldx * 2);
    m->h.ensure((size_t)M * ldh * 2);
    bf16_t *qh = m->q.as<bf16_t>(), *kh = m->vt_pre.as<bf16_t>(), *vh = kh + 2 * kplane;
    // folded RMSNorm as in run_prefill_layers (opt-in): the producer writes both planes of xg ([hi | lo], the lo plane D columns right)
    FoldRun fr = fold_run(m, prefill_fold_on(), ldx, D);
    auto mm = [&](const bf16_t* A, int lda, const bf16_t* W, void* out, int N, int K, int ldo, int epi, int lo_off, const NormFold* fold) {
        gemm_split(m, A, W, nullptr, out, M, N, K, ldo, epi, lda, lo_off, fold);
    };
    auto norm = [&](const float* w) { launch_rmsnorm_split(m->x.as<float>(), nullptr, w, m->xn.as<bf16_t>(), M, D, c.rms_eps, ldx, D, m->st); };
    for (int l = l0; l < nl; ++l) {
        const LlmLayer& L = m->llm[l];
        if (!fr.have_xg) norm(L.in_norm);
        mm(m->xn.as<bf16_t>(), ldx, L.qkv_w, m->s_qkv.p, 3 * D, D, 3 * D, EPI_F32, 0, fr.have_xg ? &fr.cons : nullptr);
        QkvSplit32Args qa{m->s_qkv.as<float>(), qh, qh + qplane, kh, kh + kplane, vh, vh + kplane,
                          reinterpret_cast<float*>(kcache(m, kv, l)), reinterpret_cast<float*>(vcache(m, kv, l)),
                          B, S, H, m->hd, S, Sr, Sr, kv.capS, m->rope_cos, m->rope_sin, kv.es == 3};
        launch_qkv_split32(qa, m->st);
        AttnArgs aa{qh, kh, vh, m->attn.as<bf16_t>(), B, H, S, m->hd, S, Sr, 1, 1.0f / sqrtf((float)m->hd), Sr,
                    qh + qplane, kh + kplane, vh + kplane, ldx, D};
        attach_kmask(m, aa, m->has_kmask);
        launch_attention(aa, m->st);
        if (m->attn_out) {
            AttnProbsArgs pa{};
            pa.q_hi = qh;
            pa.q_lo = qh + qplane;
            pa.k_hi = kh;
            pa.k_lo = kh + kplane;
            pa.q_stride = S;
            pa.kv_stride = Sr;
            emit_attentions(m, l, B, S, pa);
        }
        layer_tail_on(m, L, M, TailLd{ldx, ldx, ldh, F}, mm, norm, fr, l + 1 < nl ? m->llm[l + 1].in_norm : nullptr);
        emit_hidden(m, l + 1, B, S);
    }
}

// ---- one cached decode step over the first `nrows` rows of a loop (captured into a hipGraph): 5 launches per layer + 2.
// x_dec (fp32 residual rows of the new tokens), their sum-of-squares partials and xg are prepared by the previous step's
// select kernel (or by embed_tokens_ssq when the host supplies the tokens).  Positions, step counts and every
// generation parameter are read from the rows' RowState records.
SelectArgs select_args(vc_model* m, const LoopView& v, const float* logits, int nrows, int advance) {
    SelectArgs a{};
    a.logits = logits;
    a.ldl = m->c.vocab;
    a.rows = v.rows;
    a.next_tok = v.next_tok;
    a.out_ids = v.out_ids;
    a.embed = m->embed;
    a.embed_lo = (m->precision || v.split_G) ? lo_plane(m, m->embed) : nullptr;   // strict / split on an inexact checkpoint: x = hi + lo
    a.x = v.x_dec;
    a.ssq = v.ssq;
    a.xg_w = m->llm[0].in_norm;
    a.xg = v.xg_dec;
    a.D = m->c.hidden;
    a.npart = m->npart;
    a.V = m->c.vocab;
    a.nrows = nrows;
    a.advance = advance;
    a.xg_G = v.split_G;
    return a;
}

// log-prob of the token the selection just chose + the loop's lp_k most likely tokens, into the row's slot of the slabs: right behind
// launch_select_embed, on the same logits (the raw distribution, whatever the sampler made of it).  Nothing without slabs.
void enqueue_step_logprobs(vc_model* m, const LoopView& v, const float* logits, int nrows) {
    if (!v.lp_tok) return;
    TopkLogprobArgs a{logits, m->c.vocab, nullptr, v.lp_tok, v.lp_top, v.lp_ids, m->c.vocab, v.lp_k, v.rows, v.next_tok, 0};
    launch_topk_logprob(a, nrows, -1, v.st);
}

// the logits processors of the loop's rows in front of the selection: -> the rows launch_select_embed reads (the raw ones without a
// request: nothing is launched).  enqueue_step_logprobs keeps reading the raw rows.
const float* enqueue_step_processors(vc_model* m, const LoopView& v, const float* logits, int nrows) {
    if (!v.proc_logits) return logits;
    LogitsProcessArgs a{logits, m->c.vocab, v.proc_logits, m->c.vocab, v.rows, v.proc_prompt, v.out_ids, v.proc_bad, m->c.vocab};
    a.cn_state_off = v.cn_state_off;   // (nullptr / 0 without a token automaton)
    a.cn_edge_tok = v.cn_edge_tok;
    a.cn_edge_next = v.cn_edge_next;
    a.cn_default_next = v.cn_default_next;
    a.cn_states = v.cn_states;
    launch_logits_process(a, nrows, v.st);
    return v.proc_logits;
}

// the selection tail of a step on `logits`: the processors (a view with their buffers), the selection + embedding of the chosen
// tokens (K19/K20+K10), the log-probs (a view with slabs).  advance 3: a cached step; 1: step 0 on the prefill logits.
// A guided view (gd_logits; vc_request_guidance): nrows = 2 B — the raw rows of the B conditional sequences, then those of their
// followers.  combine (B pairs -> the guided rows) | the processors on the guided rows | selection + embedding for the B conditional
// rows | follow (the followers take the chosen tokens and advance their own positions) | the log-probs of the RAW conditional rows.
void enqueue_selection(vc_model* m, const LoopView& v, const float* logits, int nrows, int advance) {
    if (v.gd_logits) {
        const int B = nrows / 2, V = m->c.vocab;
        GuidanceCombineArgs ca{logits, logits + (size_t)B * V, V, v.gd_logits, V, v.rows, v.gd_scalars, V};
        launch_guidance_combine(ca, B, v.st);
        launch_select_embed(select_args(m, v, enqueue_step_processors(m, v, v.gd_logits, B), B, advance), v.st);
        GuidanceFollowArgs fa{v.rows, v.next_tok, v.x_dec, v.ssq, v.xg_dec, B, m->c.hidden, m->npart, advance};
        launch_guidance_follow(fa, v.st);
        enqueue_step_logprobs(m, v, logits, B);
        return;
    }
    launch_select_embed(select_args(m, v, enqueue_step_processors(m, v, logits, nrows), nrows, advance), v.st);
    enqueue_step_logprobs(m, v, logits, nrows);
}

// ---- the device beam loop (vc_generate_beam) -----------------------------------------------------------------------------------
constexpr int BEAM_CAND = VC_BEAM_MAX_ROWS * VC_MAX_TOP_LOGPROBS;
constexpr int BEAM_STATE_INTS = 2 * BEAM_CAND + 3 * VC_BEAM_MAX_ROWS + VC_BEAM_MAX_ROWS * (BQ_STRIDE + BH_STRIDE) + BP_STRIDE + 4;
// bytes one (row, head) of the tail-permute staging holds: the cache rows of cap_new positions
size_t beam_span_cap(const vc_model* m, int cap_new) { return (size_t)cap_new * m->hd * m->kv_es; }
BeamLoop beam_view(vc_model* m, int B, int n) {
    BeamLoop bl{};
    int* p = m->bm_state.as<int>();
    bl.cand_lp = reinterpret_cast<float*>(p);
    bl.cand_id = p + BEAM_CAND;
    p += 2 * BEAM_CAND;
    bl.score = reinterpret_cast<float*>(p);
    bl.perm = p + VC_BEAM_MAX_ROWS;
    bl.start = p + 2 * VC_BEAM_MAX_ROWS;
    bl.seq = p + 3 * VC_BEAM_MAX_ROWS;
    bl.hyp = bl.seq + VC_BEAM_MAX_ROWS * BQ_STRIDE;
    bl.params = bl.hyp + VC_BEAM_MAX_ROWS * BH_STRIDE;
    bl.flags = bl.params + BP_STRIDE;
    bl.cap_new = m->bm_cap_new;
    bl.tmp = m->bm_tmp.p;
    bl.span_cap = beam_span_cap(m, bl.cap_new);
    bl.tok_tab = m->bm_tab.as<int>();
    bl.parent_tab = bl.tok_tab + (size_t)bl.cap_new * VC_BEAM_MAX_ROWS;
    bl.hyp_den = m->bm_den.as<float>();
    bl.done_den = bl.hyp_den + bl.cap_new + 1;
    bl.B = B;
    bl.n = n;
    return bl;
}
// the buffers of a call of R rows and max_new steps (beam_view hands their pointers and the capacity to the step)
void ensure_beam(vc_model* m, int R, int max_new) {
    m->bm_state.ensure((size_t)BEAM_STATE_INTS * 4, true);
    const int cap_new = std::max((int)rup(max_new, 64), m->bm_cap_new);
    m->bm_tab.ensure((size_t)2 * cap_new * VC_BEAM_MAX_ROWS * 4);
    m->bm_den.ensure((size_t)2 * (cap_new + 1) * 4);
    m->bm_tmp.ensure((size_t)2 * R * m->c.heads * beam_span_cap(m, cap_new));
    m->bm_cap_new = cap_new;
}
// the tail of a beam step on `logits`: the 2 n best log-probs of every row, the selection / bookkeeping kernel, the tail permute of
// every layer's K and V (`permute`; nothing to move behind the prefill) and the embedding of the chosen tokens
void enqueue_beam_tail(vc_model* m, const LoopView& v, const BeamLoop& bl, const float* logits, int advance, bool permute) {
    const vc_model_cfg& c = m->c;
    const int R = bl.B * bl.n;
    TopkLogprobArgs ta{logits, c.vocab, nullptr, nullptr, bl.cand_lp, bl.cand_id, c.vocab, 2 * bl.n, nullptr, nullptr, 0};
    launch_topk_logprob(ta, R, -1, v.st);
    BeamStepArgs ba{bl.cand_lp, bl.cand_id, bl.score, v.rows, v.next_tok, bl.perm, bl.tok_tab, bl.parent_tab, bl.seq, bl.hyp,
                    bl.hyp_den, bl.done_den, bl.params, bl.flags, bl.B, bl.n, advance};
    launch_beam_step(ba, v.st);
    if (permute) {
        const KvTarget kv = loop_kv(v);
        const int pos_bytes = m->hd * v.es;
        for (int l = 0; l < c.layers; ++l)
            launch_kv_permute_tail(kcache(m, kv, l), vcache(m, kv, l), bl.tmp, bl.perm, bl.start, v.rows, R, c.heads,
                                   (size_t)v.capS * pos_bytes, pos_bytes, bl.span_cap, v.st);
    }
    launch_embed_tokens_ssq(v.next_tok, m->embed, v.x_dec, v.ssq, m->llm[0].in_norm, v.xg_dec, R, c.hidden, m->npart, v.st, v.split_G,
                            (m->precision || v.split_G) ? lo_plane(m, m->embed) : nullptr);
}

// the fused decode attention of layer l of a step over the first `nrows` rows of a loop
AttnDecodeFusedArgs decode_attn_args(const vc_model* m, const LoopView& v, int l, int nrows) {
    const KvTarget kv = loop_kv(v);
    // AttnDecodeFusedArgs::kv32: the split step over fp24 / fp32 rows, the bf16 step over e4m3 / bf16 rows
    const int cache_format = v.split_G ? (v.es == 3 ? 2 : 1) : (v.es == 1 ? 3 : 0);
    AttnDecodeFusedArgs da{v.qkv_dec, kcache(m, kv, l), vcache(m, kv, l), v.attn_dec, nrows, m->c.heads, m->hd, v.capS,
                           v.rows + RS_POS, m->rope_cos, m->rope_sin, 1.0f / sqrtf((float)m->hd), RS_STRIDE,
                           v.rows + RS_ACTIVE, cache_format, v.split_G, v.kmask, v.kmask_stride};
    return da;
}

// hook_pos >= 0 (the rows' position): the same step run eagerly and unstamped with the output_hidden_states / output_attentions
// hooks of a cached decode step (vc_request_hidden_states / vc_request_attentions before vc_decode_step): inputs_embeds row, every
// layer's residual row, the final norm; and per layer the probabilities of the new token's query over the pos + 1 keys, recomputed
// from the step's own roped q (rounded as the fused kernel rounds it) and the K cache — the fused decode attention keeps only
// unnormalised scores.
// beam != nullptr: a step of the device beam loop — the same linears and attention, the beam tail in place of the selection.
void enqueue_decode_step(vc_model* m, const LoopView& view, int nrows, int hook_pos = -1, const BeamLoop* beam = nullptr) {
    const vc_model_cfg& c = m->c;
    const bool hooks = hook_pos >= 0;
    LoopView v = view;
    if (hooks) v.stamps = nullptr;   // next_stamp(v) == nullptr for every launch
    if (hooks) emit_hidden(m, 0, nrows, 1, v.x_dec);
    decode_linears(
        m, v, nrows,
        [&](int l) {
            AttnDecodeFusedArgs da = decode_attn_args(m, v, l, nrows);
            da.stamp = next_stamp(v);
            if (v.fan_n > 1) {   // rows g n .. g n + n - 1 over the prompt keys of cache row g, read once per (group, head)
                AttnFanoutArgs fa{v.qkv_dec, da.k, da.v, v.attn_dec, nrows / v.fan_n, c.heads, m->hd, v.capS, v.fan_n, v.capR, v.rows + RS_POS,
                                  RS_STRIDE, v.fan_P, nullptr, m->rope_cos, m->rope_sin, da.scale, v.es == 1 ? 3 : 0};
                launch_attention_fanout(fa, v.st);
            } else {
                launch_attention_decode_fused(da, v.st);
            }
            if (hooks && m->attn_out) {
                m->attn_q.ensure((size_t)nrows * c.hidden * 4);
                launch_rope_q_decode(v.qkv_dec, v.split_G != 0, m->attn_q.as<float>(), nrows, c.heads, m->hd, hook_pos, m->rope_cos,
                                     m->rope_sin, v.split_G == 0, v.st);
                const bf16_t* k = da.k;
                AttnProbsArgs pa{};
                pa.q32 = m->attn_q.as<float>();
                if (v.split_G && v.es == 3) pa.k24 = k;
                else if (v.split_G) pa.k32 = reinterpret_cast<const float*>(k);
                else if (v.es == 1) pa.k8 = reinterpret_cast<const uint8_t*>(k);   // the fp8 weight format's e4m3 rows
                else pa.k_hi = k;
                pa.q_stride = 1;
                pa.kv_stride = v.capS;
                emit_attentions(m, l, nrows, 1, pa, hook_pos + 1, hook_pos);
            }
        },
        [&](int l) {
            if (hooks) emit_hidden(m, l + 1, nrows, 1, v.x_dec);
        });
    if (beam) enqueue_beam_tail(m, v, *beam, v.logits, 3, true);
    else enqueue_selection(m, v, v.logits, nrows, 3);
    // in-situ timing: fold the step's slots (5 per layer: qkv, attention, o, gate/up, down; then lm_head) into the span's sums
    if (v.stamps && v.stamp_next && v.prof_acc)
        launch_stamp_accumulate(v.stamps, *v.stamp_next, m->c.layers, v.prof_acc, v.stamp_scratch, v.st);
}

// strict mode: the rows of a session advance in lockstep, so row 0's position serves every row of the fp32 kernels — except behind a
// guided vc_prefill (gd_pair), whose pairs stand at different positions: every row then reads its own record
void enqueue_decode_step_strict(vc_model* m, const LoopView& v, int B) {
    emit_hidden(m, 0, B, 1, m->x_dec.as<float>());
    run_llm_layers_strict(m, m->x_dec.as<float>(), B, 1, v.rows + RS_POS, false, 0, m->gd_pair ? RS_STRIDE : 0);
    logits_strict(m, m->x_dec.as<float>(), nullptr, B);
    enqueue_selection(m, v, v.logits, B, 3);
}

// ---- logits of precision mode 0 from the residual rows x (B sequences of rows_per_seq rows) --------------------------------------
// final norm of each sequence's last row -> lm_head GEMV -> m->logits [B, V]
void last_row_logits(vc_model* m, const float* x, int B, int rows_per_seq) {
    const vc_model_cfg& c = m->c;
    std::vector<int> idx(B);
    for (int b = 0; b < B; ++b) idx[b] = b * rows_per_seq + rows_per_seq - 1;
    HIPCHK(hipMemcpyAsync(m->last_idx.p, idx.data(), B * 4, hipMemcpyHostToDevice, m->st));
    launch_rmsnorm_rows(x, m->last_idx.as<int>(), m->final_norm, m->xl.as<bf16_t>(), B, c.hidden, c.rms_eps, m->st);
    LoopView lv{};  // the lm_head GEMV over the last rows only needs a stream
    lv.st = m->st;
    gemv(m, lv, m->xl.as<bf16_t>(), m->lm_head_p, nullptr, m->logits.p, B, c.vocab, c.hidden, c.vocab, GEMV_F32);
    HIPCHK(hipStreamSynchronize(m->st));   // `idx` is host memory
}
// final norm -> lm_head GEMM over all M rows -> m->logits_all [M, V] (sized by the caller)
void all_row_logits(vc_model* m, const float* x, int M) {
    const vc_model_cfg& c = m->c;
    launch_rmsnorm(x, m->final_norm, m->xn.as<bf16_t>(), M, c.hidden, c.rms_eps, m->st);
    gemm(m, m->xn.as<bf16_t>(), m->lm_head, nullptr, m->logits_all.p, M, c.vocab, c.hidden, c.vocab, EPI_F32);
}

// ---- multi-token continuation of the session's cached rows (vc_extend), precision mode 0 ----------------------------------
// M = B n new rows (row b n + t = token t of sequence b at position P + t).  Per layer: QKV projection -> RoPE at P + t and the
// K / V rows written into the cache at P + t (qkv_split_kernel over pointers advanced by P rows: its RoPE table and cache
// rows are indexed by t) -> attention_extend over the cache -> o / gate-up / down.  The linears run on the decode GEMVs (one
// weight pass per 32 rows, folded RMSNorm) up to EXTEND_GEMV_ROWS rows, above that on the prefill GEMMs (W8A8 for the fp8
// format).  Leaves the residual rows in `x_out` (m->x) and logits of every row in m->logits_all when all_rows, else of each
// sequence's last row in m->logits.
// Crossover measured on MI355X (tools/kbench.py extend_linears, one 7b layer's qkv / o / gate-up / down, bf16): ceil(M / 32)
// GEMV passes against one GEMM per matrix = 90 / 174 / 264 / 351 / 436 us against 343 / 350 / 354 / 358 / 351 us at
// M = 32 / 64 / 96 / 128 / 160 (profiles/extend_wall_times.md): the GEMV passes win up to 128 rows.
constexpr int EXTEND_GEMV_ROWS = 128;
void run_extend(vc_model* m, const int* tok_dev, int B, int n, bool all_rows) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn, H = c.heads, M = B * n, P = m->cur_pos, hd = m->hd;
    const KvTarget kv = session_kv(m);
    const bool kv8 = kv.es == 1, f8 = m->weight_format == 2;
    const bool use_gemv = M <= EXTEND_GEMV_ROWS;
    const int nr = (int)rup(n, 64);
    // workspaces: the prefill's buffers, which no captured decode graph refers to
    m->x.ensure((size_t)M * D * 4);
    m->xn.ensure((size_t)M * (D + XN_PAD) * 2);
    m->qkv.ensure((size_t)M * 3 * D * 2);
    m->q.ensure((size_t)M * D * 2);
    m->attn.ensure((size_t)M * D * 2);
    m->h.ensure((size_t)M * F * 2);
    m->p_ssq.ensure((size_t)M * m->npart * 4);
    m->vt_pre.ensure((size_t)B * H * hd * nr * 2);   // V^T rows qkv_split writes for a flash kernel (unused here)
    if (kv8) m->k_pre.ensure((size_t)B * H * nr * hd * 2);
    if (f8 && !use_gemv) {
        m->a8.ensure((size_t)M * std::max(D, F));
        m->a8_scale.ensure((size_t)M * 4);
    }
    if (all_rows || use_gemv) m->logits_all.ensure((size_t)M * c.vocab * 4);
    float* x = m->x.as<float>();
    auto attention = [&](int l, const bf16_t* qkv_rows) {
        // RoPE at P + t, K / V rows into the cache at P + t (bf16, or e4m3 with the bf16 K rows in a scratch)
        const size_t off = (size_t)P * hd;
        QkvSplitArgs qa{qkv_rows, m->q.as<bf16_t>(), kv8 ? m->k_pre.as<bf16_t>() : kcache(m, kv, l) + off, m->vt_pre.as<bf16_t>(),
                        B, n, H, hd, n, kv8 ? nr : kv.capS, nullptr, m->rope_cos + off / 2, m->rope_sin + off / 2,
                        kv8 ? nullptr : vcache(m, kv, l) + off, nr,
                        kv8 ? reinterpret_cast<uint8_t*>(kcache(m, kv, l)) + off : nullptr,
                        kv8 ? reinterpret_cast<uint8_t*>(vcache(m, kv, l)) + off : nullptr, kv.capS};
        launch_qkv_split(qa, m->st);
        AttnExtendArgs ea{m->q.as<bf16_t>(), kcache(m, kv, l), vcache(m, kv, l), m->attn.as<bf16_t>(), B, H, n, P, hd, n, kv.capS,
                          kv8 ? 1 : 0, 1.0f / sqrtf((float)hd), nullptr, 0};
        attach_kmask(m, ea, m->kmask_in_decode);
        launch_attention_extend(ea, m->st);
        if (m->attn_out) {
            AttnProbsArgs pa{};
            pa.q_hi = m->q.as<bf16_t>();
            if (kv8) pa.k8 = reinterpret_cast<const uint8_t*>(kcache(m, kv, l));
            else pa.k_hi = kcache(m, kv, l);
            pa.q_stride = n;
            pa.kv_stride = kv.capS;
            emit_attentions(m, l, B, n, pa, P + n, P);
        }
    };
    if (use_gemv) {
        // the decode step's GEMVs over M rows (gemv() runs one weight pass per 32 rows)
        LoopView v{};
        v.st = m->st;
        v.x_dec = x;
        v.xg_dec = m->xn.as<bf16_t>();
        v.qkv_dec = m->qkv.as<bf16_t>();
        v.attn_dec = m->attn.as<bf16_t>();
        v.h_dec = m->h.as<bf16_t>();
        v.logits = m->logits_all.as<float>();
        v.ssq = m->p_ssq.as<float>();
        v.sk_scratch = m->sk_scratch.as<float>();
        v.sk_counters = m->sk_counters.as<unsigned>();
        launch_embed_tokens_ssq(tok_dev, m->embed, x, v.ssq, m->llm[0].in_norm, v.xg_dec, M, D, m->npart, m->st);
        emit_hidden(m, 0, B, n, x);
        decode_linears(m, v, M, [&](int l) { attention(l, v.qkv_dec); }, [&](int l) { emit_hidden(m, l + 1, B, n, x); });
        return;
    }
    launch_embed_tokens(tok_dev, m->embed, x, M, D, m->st);
    emit_hidden(m, 0, B, n, x);
    FoldRun fr;   // (a continuation never folds its norms)
    for (int l = 0; l < c.layers; ++l) {
        const LlmLayer& L = m->llm[l];
        qkv_projection(m, L, M, fr);
        attention(l, m->qkv.as<bf16_t>());
        layer_tail(m, L, M, fr, nullptr);
        emit_hidden(m, l + 1, B, n, x);
    }
    if (all_rows) all_row_logits(m, x, M);
    else last_row_logits(m, x, B, n);   // the last row of every sequence through the lm_head GEMV, as a prefill does
}

hipGraphExec_t capture_step(vc_model* m, const LoopView& v, int nrows, const BeamLoop* beam = nullptr) {
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    // thread-local mode: other sessions (host threads) may allocate / copy while this thread captures
    HIPCHK(hipStreamBeginCapture(v.st, hipStreamCaptureModeThreadLocal));
    try {
        enqueue_decode_step(m, v, nrows, -1, beam);
    } catch (...) {
        (void)hipStreamEndCapture(v.st, &g);
        throw;
    }
    HIPCHK(hipStreamEndCapture(v.st, &g));
    HIPCHK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(g));
    return exec;
}

// the session's captured step of `kind` for this view, row count and (a beam step) beam loop: the one it holds if it was captured from
// an equal description (StepKey), else a new capture in its place
hipGraphExec_t step_graph(vc_model* m, StepKind kind, const LoopView& view, int nrows, const BeamLoop* beam = nullptr) {
    StepGraph& s = m->step[kind];
    const StepKey key{view, nrows, beam != nullptr, beam ? *beam : BeamLoop{}};
    if (s.exec && s.key == key) return s.exec;
    if (s.exec) {
        (void)hipGraphExecDestroy(s.exec);
        s.exec = nullptr;
    }
    s.exec = capture_step(m, view, nrows, beam);
    s.key = key;
    m->step_captures += 1;
    return s.exec;
}

// ---- prompt-lookup speculation: the verify step (STEP_SPEC) ---------------------------------------------------------------------
// device words of sp_state: query counts | counters | prompt lengths | lookup lengths, VC_MAX_ROWS sequences each
constexpr int SPEC_STATE_INTS = VC_MAX_ROWS * (1 + 4 + 1 + 1);
constexpr int SPEC_MAX_ROWS = VC_GEMV_MAX_M;   // B * (k + 1) rows ride one weight pass
// the buffers of a speculated call of B sequences, Q rows each: the per-step buffers of R = B * Q rows, the id stores (strides
// max_positions: no call's lengths are baked into the step), the log-prob scratch of the widest K; any: the selections and their
// log-probs; proc: the processed rows of the verify form of the processors
void ensure_spec(vc_model* m, int R, bool any = false, bool proc = false) {
    const vc_model_cfg& c = m->c;
    const size_t Rp = rup(R, 16), D = c.hidden;
    m->sp_x.ensure(Rp * D * 4, true);
    m->sp_xg.ensure(Rp * D * 2, true);
    m->sp_qkv.ensure(Rp * 3 * D * 2, true);
    m->sp_attn.ensure(Rp * D * 2, true);
    m->sp_h.ensure(Rp * c.ffn * 2, true);
    m->sp_logits.ensure(Rp * c.vocab * 4, true);
    m->sp_ssq.ensure(Rp * m->npart * 4, true);
    m->sp_tok.ensure((size_t)SPEC_MAX_ROWS * 4, true);
    m->sp_state.ensure((size_t)SPEC_STATE_INTS * 4, true);
    m->sp_lookup.ensure((size_t)VC_MAX_ROWS * c.max_positions * 4);
    m->sp_prompt.ensure((size_t)VC_MAX_ROWS * c.max_positions * 4);
    m->sp_lp.ensure((size_t)SPEC_MAX_ROWS * VC_MAX_TOP_LOGPROBS * 4);
    m->sp_ids.ensure((size_t)SPEC_MAX_ROWS * VC_MAX_TOP_LOGPROBS * 4);
    if (any) {
        m->sp_sel.ensure((size_t)SPEC_MAX_ROWS * 4, true);
        m->sp_chosen.ensure((size_t)SPEC_MAX_ROWS * 4, true);
    }
    if (any && proc) m->sp_proc.ensure(Rp * c.vocab * 4, true);
}
SpecLoop spec_view(vc_model* m, int B, int Q, int ngram, bool lookup, int lp_k, bool any = false, bool proc = false) {
    SpecLoop sl{};
    int* st = m->sp_state.as<int>();
    sl.tok = m->sp_tok.as<int>();
    sl.nq = st;
    sl.counters = st + VC_MAX_ROWS;
    sl.prompt_len = st + 5 * VC_MAX_ROWS;
    sl.prompt = m->sp_prompt.as<int>();
    sl.prompt_stride = m->c.max_positions;
    if (lookup) {
        sl.lookup = m->sp_lookup.as<int>();
        sl.lookup_len = st + 6 * VC_MAX_ROWS;
        sl.lookup_stride = m->c.max_positions;
    }
    if (lp_k >= 0) {   // a call with log-probs: entry 0 of a scratch row is the row's argmax
        sl.s_lp = m->sp_lp.as<float>();
        sl.s_ids = m->sp_ids.as<int>();
        sl.s_k = std::max(lp_k, 1);
    }
    if (any) {   // the wider scope: the rows are selected by launch_spec_select (on processed rows with a processor set)
        sl.sel = m->sp_sel.as<int>();
        if (lp_k >= 0) sl.s_chosen = m->sp_chosen.as<float>();
        if (proc) sl.proc_out = m->sp_proc.as<float>();
    }
    sl.B = B;
    sl.Q = Q;
    sl.ngram = ngram;
    return sl;
}
// the per-step buffers of a view replaced by the B * Q row ones (the caches, records, next_tok, out_ids and slabs stay)
LoopView spec_loop_view(vc_model* m, const LoopView& call) {
    LoopView v = call;
    v.x_dec = m->sp_x.as<float>();
    v.xg_dec = m->sp_xg.as<bf16_t>();
    v.qkv_dec = m->sp_qkv.as<bf16_t>();
    v.attn_dec = m->sp_attn.as<bf16_t>();
    v.h_dec = m->sp_h.as<bf16_t>();
    v.logits = m->sp_logits.as<float>();
    v.ssq = m->sp_ssq.as<float>();
    return v;
}
// draft + embedding of the B * Q token rows -> the linears with the verify attention between -> (the wider scope: the processors'
// verify form, the rows' selections) -> (log-probs of every row, always of the raw rows) -> accept
void enqueue_spec_step(vc_model* m, const LoopView& v, const SpecLoop& sl) {
    const vc_model_cfg& c = m->c;
    const int R = sl.B * sl.Q;
    SpecDraftArgs da{v.rows, v.out_ids, sl.lookup, sl.lookup_len, sl.lookup_stride, sl.prompt, sl.prompt_len, sl.prompt_stride,
                     sl.tok, sl.nq, sl.B, sl.Q, sl.Q - 1, sl.ngram, c.vocab};
    launch_spec_draft(da, v.st);
    launch_embed_tokens_ssq(sl.tok, m->embed, v.x_dec, v.ssq, m->llm[0].in_norm, v.xg_dec, R, c.hidden, m->npart, v.st);
    const KvTarget kv = loop_kv(v);
    decode_linears(m, v, R, [&](int l) {
        AttnVerifyArgs va{v.qkv_dec, kcache(m, kv, l), vcache(m, kv, l), v.attn_dec, sl.B, c.heads, m->hd, v.capS, sl.Q,
                          v.rows + RS_POS, RS_STRIDE, sl.nq, m->rope_cos, m->rope_sin, 1.0f / sqrtf((float)m->hd), v.es == 1 ? 3 : 0,
                          v.kmask, v.kmask_stride};
        launch_attention_verify(va, v.st);
    });
    if (sl.sel) {
        const float* lg = v.logits;
        if (sl.proc_out) {
            LogitsProcessArgs pa{v.logits, c.vocab, sl.proc_out, c.vocab, v.rows, v.proc_prompt, v.out_ids, v.proc_bad, c.vocab, sl.Q, sl.tok, sl.nq};
            launch_logits_process(pa, R, v.st);
            lg = sl.proc_out;
        }
        SpecSelectArgs sa{lg, c.vocab, c.vocab, v.rows, sl.nq, sl.sel, sl.B, sl.Q, 0};
        launch_spec_select(sa, -1, v.st);
    }
    if (v.lp_tok) {   // (rows behind a sequence's queries hold a stale selection: any id, scored and never read)
        TopkLogprobArgs ta{v.logits, c.vocab, sl.sel, sl.s_chosen, sl.s_lp, sl.s_ids, c.vocab, sl.s_k, nullptr, nullptr, 0};
        launch_topk_logprob(ta, R, -1, v.st);
    }
    SpecAcceptArgs aa{v.logits, c.vocab, c.vocab, v.rows, v.next_tok, v.out_ids, sl.tok, sl.nq, sl.B, sl.Q, sl.counters,
                      v.lp_tok ? sl.s_lp : nullptr, v.lp_tok ? sl.s_ids : nullptr, sl.s_k, v.lp_tok, v.lp_top, v.lp_ids, v.lp_k,
                      sl.sel, v.lp_tok ? sl.s_chosen : nullptr};
    launch_spec_accept(aa, v.st);
}
// the session's captured verify step for this view and loop: replayed while both equal what it was captured from
hipGraphExec_t spec_step_graph(vc_model* m, const LoopView& view, const SpecLoop& sl) {
    StepGraph& s = m->step[STEP_SPEC];
    StepKey key{view, sl.B * sl.Q, false, BeamLoop{}, sl};
    if (s.exec && s.key == key) return s.exec;
    if (s.exec) {
        (void)hipGraphExecDestroy(s.exec);
        s.exec = nullptr;
    }
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(view.st, hipStreamCaptureModeThreadLocal));
    try {
        enqueue_spec_step(m, view, sl);
    } catch (...) {
        (void)hipStreamEndCapture(view.st, &g);
        throw;
    }
    HIPCHK(hipStreamEndCapture(view.st, &g));
    HIPCHK(hipGraphInstantiate(&s.exec, g, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(g));
    s.key = key;
    m->step_captures += 1;
    return s.exec;
}

void ensure_out_ids(vc_model* m, int B, int max_new) {
    const int stride = std::max(max_new, 1);
    if (stride > m->out_stride || m->out_ids.cap < (size_t)rup(B, 16) * stride * 4) {
        m->out_stride = std::max(stride, m->out_stride);
        m->out_ids.ensure((size_t)rup(B, 16) * m->out_stride * 4);
    }
}
// the log-prob slabs of a generate() call, sized like out_ids (after ensure_out_ids): [rows, out_stride] (x K)
void ensure_logprob_slabs(vc_model* m, int B, int K) {
    const size_t slots = (size_t)rup(B, 16) * m->out_stride;
    m->lp_tok.ensure(slots * 4);
    m->lp_top.ensure(slots * std::max(K, 1) * 4);
    m->lp_ids.ensure(slots * std::max(K, 1) * 4);
}

// the buffers of a generate() call with logits processors: the prompt ids [B, T], the bad-word table, the processed rows [B, V]
void ensure_processor_buffers(vc_model* m, int B, int T) {
    m->proc_prompt.ensure((size_t)B * T * 4);
    m->proc_bad.ensure((size_t)VC_MAX_BAD_WORDS * (1 + VC_MAX_BAD_WORD_LEN) * 4);
    m->proc_logits.ensure((size_t)rup(B, 16) * m->c.vocab * 4);
}

// ---- host-side RowState records ---------------------------------------------------------------------------------
struct GenParams {  // what a generate() call asks for (HF GenerationMixin subset; SURVEY.md Appendix C)
    int max_new = 0, eos = -1, pad = 0;
    int do_sample = 0, top_k = 0;
    float temperature = 1.f, top_p = 1.f;
    float min_p = 0.f, typical_p = 0.f, epsilon_cutoff = 0.f, eta_cutoff = 0.f;   // vc_request_sampling_warpers; 0: off
    uint64_t seed = 0;
    int n_stop = 0;
    int stop[VC_MAX_STOP][1 + VC_MAX_STOP_LEN] = {};
    // logits processors (vc_request_logits_processors; proc 0: the RS_LP_* slots stay zero); row b's prompt ids are ids[b * proc_T ..]
    int proc = 0, proc_ngram = 0, proc_minnew = 0, proc_nbad = 0, proc_neos = 0, proc_T = 0;
    float proc_penalty = 1.f;
    int proc_eos[VC_MAX_EOS_EXTRA] = {};
    int cn = 0;   // a token automaton masks the rows (vc_request_constraint): RS_CN_ON; implies proc — the launch that carries it
};

uint32_t mix_seed(uint64_t seed, uint32_t row, uint32_t salt) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(row + 1) + salt;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

// records of the B rows of one request (row b of the request = record b); `tail` = last prompt ids per row, right-aligned
// fan > 1 (a served vc_request_fanout): B = prompts x fan rows; row b continues prompt b / fan — its stop-sequence tail and its
// processor history are that prompt's, its seed and its out_ids slot its own
void fill_rows(int* rec, int B, const GenParams& g, int pos, const int* tail /*[B / fan][VC_MAX_STOP_LEN-1] or null*/, int out_off0,
               int out_stride, int fan = 1) {
    memset(rec, 0, (size_t)B * RS_STRIDE * sizeof(int));
    const float inv_t = 1.0f / g.temperature;
    for (int b = 0; b < B; ++b) {
        int* r = rec + (size_t)b * RS_STRIDE;
        r[RS_ACTIVE] = 1;
        r[RS_POS] = pos;
        r[RS_MAXNEW] = g.max_new;
        r[RS_EOS] = g.eos;
        r[RS_PAD] = g.pad;
        r[RS_NSTOP] = g.n_stop;
        r[RS_SAMPLE] = g.do_sample;
        memcpy(&r[RS_INVTEMP], &inv_t, 4);
        r[RS_TOPK] = g.top_k;
        memcpy(&r[RS_TOPP], &g.top_p, 4);
        memcpy(&r[RS_MINP], &g.min_p, 4);
        memcpy(&r[RS_TYPICAL], &g.typical_p, 4);
        memcpy(&r[RS_EPS], &g.epsilon_cutoff, 4);
        memcpy(&r[RS_ETA], &g.eta_cutoff, 4);
        r[RS_SEED_LO] = (int)mix_seed(g.seed, (uint32_t)b, 0x51u);  // per-row streams: independent of the row's slot
        r[RS_SEED_HI] = (int)mix_seed(g.seed, (uint32_t)b, 0xA7u);
        r[RS_OUT_OFF] = out_off0 + b * out_stride;
        for (int j = 0; j < VC_MAX_STOP_LEN - 1; ++j) r[RS_TAIL + j] = tail ? tail[(b / fan) * (VC_MAX_STOP_LEN - 1) + j] : INT32_MIN;
        for (int q = 0; q < g.n_stop; ++q)
            for (int j = 0; j < 1 + VC_MAX_STOP_LEN; ++j) r[RS_STOP + q * (1 + VC_MAX_STOP_LEN) + j] = g.stop[q][j];
        if (g.proc) {
            memcpy(&r[RS_LP_PENALTY], &g.proc_penalty, 4);
            r[RS_LP_NGRAM] = g.proc_ngram;
            r[RS_LP_MINNEW] = g.proc_minnew;
            r[RS_LP_HIST_OFF] = (b / fan) * g.proc_T;
            r[RS_LP_HIST_LEN] = g.proc_T;
            r[RS_LP_NBAD] = g.proc_nbad;
            r[RS_LP_NEOS] = g.proc_neos;
            for (int e = 0; e < g.proc_neos; ++e) r[RS_LP_EOS + e] = g.proc_eos[e];
        }
        r[RS_CN_ON] = g.cn;   // (RS_CN_STATE / RS_CN_POS zero: the start state, nothing consumed)
    }
}

// prefill through the last-row logits; leaves logits [B,V] on device
// encode + splice: inputs_embeds of the batch in m->x.  `own_kv`: size the session's own KV cache / decode loop for the
// spliced length plus reserve_new positions (reserve_new < 0: a hint, see below); otherwise only the prefill workspaces
// (the keys go to a pool's cache and the caller checks the capacity).
void do_prefill(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                int on_dev, int has_mask, int reserve_new, bool own_kv, int* S_out) {
    const vc_model_cfg& c = m->c;
    REQUIRE(m->finalized, VC_ERR_STATE, "vc_model_finalize() has not been called");
    REQUIRE(B >= 1 && T >= 1 && ids, VC_ERR_INVALID, "bad ids/B/T");
    REQUIRE(B <= VC_MAX_ROWS, VC_ERR_INVALID, "batch %d: at most %d sequences per prefill (larger batches run in pieces)", B,
            VC_MAX_ROWS);
    // images == NULL: the reference's prepare_inputs_labels_for_multimodal returns early (vcoder_ds_llava_arch.py:129-133) and
    // the call is a plain LlamaForCausalLM forward over the text ids (every id must be a vocabulary id)
    const bool text_only = img == nullptr;
    if (text_only || c.variant == VC_VARIANT_LLAVA) seg = depth = nullptr;
    if (c.variant != VC_VARIANT_VCODER_DS) depth = nullptr;
    PixSet pix{{img, seg, depth}, {0, 0, 0}};
    for (int k = 0; k < 3; ++k) {
        m->img_first[k].clear();
        if (!pix.p[k]) continue;
        if (m->img_counts[k].empty()) {
            pix.n[k] = B;
        } else {
            REQUIRE((int)m->img_counts[k].size() == B, VC_ERR_INVALID, "image counts given for %zu samples, batch is %d",
                    m->img_counts[k].size(), B);
            m->img_first[k].push_back(0);
            for (int b = 0; b < B; ++b) m->img_first[k].push_back(m->img_first[k].back() + m->img_counts[k][b]);
            pix.n[k] = m->img_first[k].back();
        }
    }
    for (auto& v : m->img_counts) v.clear();  // one-shot
    if (m->ev[0]) HIPCHK(hipEventRecord(m->ev[0], m->st));
    if (text_only) {
        for (int k = 0; k < 3; ++k) m->feat_rows[k] = 0;
        if (m->precision) m->s_feats.ensure(256);   // the fp32 splice takes a feature base pointer (no row refers to it)
        else m->feats.ensure(256);
    } else if (m->plan_only) {
        // the plan needs the feature-row COUNTS of every modality and the depth pixels (is_depth_zero), not the features
        int order[3], first_img[3];
        stage_pixels(m, pix, on_dev, order, first_img, 1u << VC_MOD_DEPTH);
        set_feat_rows(m, pix, first_img, m->Tv - (c.vit_keep_cls ? 0 : 1));
    } else if (m->precision == 1) run_vit_and_adapters_strict(m, pix, on_dev);
    else if (m->precision == 2) run_vit_and_adapters_split(m, pix, on_dev);
    else run_vit_and_adapters(m, pix, on_dev);
    const int R = m->Tv - (c.vit_keep_cls ? 0 : 1);
    std::vector<bool> dz;
    if (depth) {  // is_depth_zero = [mean(d) == 0 for d in depth_images]  (vcoder_ds_llava_arch.py:161) — one host sync, as the reference
        const int nd = pix.n[VC_MOD_DEPTH];
        m->dsum.ensure((size_t)rup(nd, 16) * ROW_SUM_PARTS * 4);
        int di = 0;
        for (int k = 0; k < 2; ++k) di += pix.n[k];
        const size_t img_elems = (size_t)3 * c.vit_image * c.vit_image;
        launch_row_sum(m->v_pixels.as<float>() + (size_t)di * img_elems, img_elems, nd, m->dsum.as<float>(), m->st);
        std::vector<float> hp((size_t)nd * ROW_SUM_PARTS), hs(nd, 0.f);
        HIPCHK(hipMemcpyAsync(hp.data(), m->dsum.p, hp.size() * 4, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        for (int i = 0; i < nd; ++i)
            for (int q = 0; q < ROW_SUM_PARTS; ++q) hs[i] += hp[(size_t)i * ROW_SUM_PARTS + q];
        const std::vector<int>& first = m->img_first[VC_MOD_DEPTH];
        for (int b = 0; b < B; ++b) {
            const int i0 = first.empty() ? b : first[b], i1 = first.empty() ? b + 1 : first[b + 1];
            float tot = 0.f;
            for (int i = i0; i < i1; ++i) tot += hs[i];
            dz.push_back(i1 > i0 && tot / ((float)(i1 - i0) * (float)img_elems) == 0.0f);
        }
    }
    if (m->ev[1]) HIPCHK(hipEventRecord(m->ev[1], m->st));
    std::vector<std::vector<RowSrc>> rows;
    const int64_t* labels = m->score_on ? m->score_labels.data() : nullptr;   // announced by vc_request_token_scores, checked by vc_prefill
    std::vector<std::vector<int64_t>> row_labels;
    if (text_only) {
        rows.assign(B, {});
        if (labels) row_labels.assign(B, {});
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t) {
                const int64_t id = ids[(size_t)b * T + t];
                REQUIRE(id >= 0 && id < c.vocab, VC_ERR_INDEX, "index out of range in self (id %lld reached the embedding lookup)",
                        (long long)id);
                rows[b].push_back({0, (int)id});
                if (labels) row_labels[b].push_back(labels[(size_t)b * T + t]);
            }
    } else {
        plan_rows(m, ids, B, T, seg != nullptr, depth ? &dz : nullptr, R, rows, labels, &row_labels);
    }
    size_t S = 0;
    bool unequal = false;
    for (auto& r : rows) {
        S = std::max(S, r.size());
        unequal |= r.size() != rows[0].size();
    }
    // quirk 6: unequal spliced lengths with an attention_mask and no labels die at vcoder_ds_llava_arch.py:295-297
    REQUIRE(!(unequal && has_mask), VC_ERR_UNEQUAL, "local variable '_new_labels' referenced before assignment");
    REQUIRE(S >= 1, VC_ERR_INVALID, "empty sequence");
    if (labels) {   // [B, S]: shorter rows are right-padded with IGNORE_INDEX (:287-293)
        m->spliced_labels.assign((size_t)B * S, IGNORE_INDEX);
        for (int b = 0; b < B; ++b) std::copy(row_labels[b].begin(), row_labels[b].end(), m->spliced_labels.begin() + (size_t)b * S);
        // what CrossEntropyLoss sees: the spliced labels behind the shift (a label the splice dropped, or at position 0, is never read).
        // Nothing of the session's cache or position has been touched yet: a refused call leaves the previous loop usable.
        for (int b = 0; b < B; ++b)
            for (size_t s = 1; s < S; ++s) {
                const int64_t l = m->spliced_labels[(size_t)b * S + s];
                REQUIRE(l == IGNORE_INDEX || (l >= 0 && l < c.vocab), VC_ERR_INDEX, "Target %lld is out of bounds.", (long long)l);
            }
        REQUIRE(m->score_cap >= (size_t)B * S, VC_ERR_INVALID,
                "token-score buffers hold %zu elements, the call yields [%d, %zu]", m->score_cap, B, S);
        REQUIRE(!m->stk_k || m->stk_cap >= (size_t)B * S * m->stk_k, VC_ERR_INVALID,
                "top-logprob buffers hold %zu entries, the call yields [%d, %zu, %d]", m->stk_cap, B, S, m->stk_k);
        if (own_kv) m->cur_pos = -1;
    }
    if (m->plan_only) {
        if (S_out) *S_out = (int)S;
        return;
    }
    // The caller's attention_mask [B, T] is LEFT-extended with "visible" over the S - T rows the splice added — by position,
    // whatever the rows hold (vcoder_ds_llava_arch.py:305-311) — and hides its zero positions as KEYS from every query of the
    // sequence in this prefill.
    std::vector<uint8_t> kmask_host;
    m->has_kmask = false;
    if (!m->mask_next.empty()) {
        std::vector<uint8_t> mk;
        mk.swap(m->mask_next);  // one-shot
        REQUIRE(m->mask_B == B && m->mask_T == T, VC_ERR_INVALID, "attention_mask is [%d, %d], input_ids [%d, %d]", m->mask_B,
                m->mask_T, B, T);
        REQUIRE((int)S >= T, VC_ERR_INVALID, "spliced length %zu shorter than the prompt %d", S, T);
        const int stride = c.max_positions, lead = (int)S - T;
        kmask_host.assign((size_t)VC_MAX_ROWS * stride, 1);
        bool any = false;
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t)
                if (!mk[(size_t)b * T + t]) {
                    kmask_host[(size_t)b * stride + lead + t] = 0;
                    any = true;
                }
        for (int b = 0; b < B && any; ++b)
            REQUIRE(kmask_host[(size_t)b * stride] != 0, VC_ERR_INVALID,
                    "attention_mask hides position 0 of sequence %d: its first queries would attend to nothing", b);
        m->has_kmask = any;
    }
    {   // reserve_new < 0: a hint (vc_prefill): as many of -reserve_new decode slots as max_position_embeddings allows;
        // reserve_new >= 0: required (generate) — exceeding max_position_embeddings is an error
        int want = (int)S + std::max(reserve_new < 0 ? -reserve_new : reserve_new, 1);
        if (reserve_new < 0) want = std::max((int)S + 1, std::min(want, c.max_positions / 64 * 64));
        if (own_kv) m->gd_pair = 0;   // (a guided vc_prefill sets it again behind its two prefills)
        if (own_kv) ensure_llm(m, std::max(B, m->fan_rows), want);   // a served fan-out / guided call: the cache and the loop of B n / 2 B rows
        else ensure_prefill_ws(m, B, (int)rup(S, 64));
    }
    std::vector<int> flat((size_t)B * S * 2);
    for (int b = 0; b < B; ++b)
        for (size_t s = 0; s < S; ++s) {
            const RowSrc r = s < rows[b].size() ? rows[b][s] : RowSrc{2, 0};  // zero right-padding (:283)
            flat[((size_t)b * S + s) * 2] = r.kind;
            flat[((size_t)b * S + s) * 2 + 1] = r.src;
        }
    HIPCHK(hipMemcpyAsync(m->row_src.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, m->st));
    if (m->has_kmask) {
        m->kmask.ensure(kmask_host.size());
        HIPCHK(hipMemcpyAsync(m->kmask.p, kmask_host.data(), kmask_host.size(), hipMemcpyHostToDevice, m->st));
    }
    m->kmask_in_decode = false;   // a decode mask never outlives its prefill (vc_prefill re-arms it)
    if (m->precision) {  // strict and split: the projected features are fp32
        if (m->precision == 1) {
            REQUIRE(own_kv, VC_ERR_STATE, "strict mode runs on the session's own decode loop");
            ensure_strict(m, std::max(B, m->fan_rows), m->capS);   // (a guided prefill: the fp32 caches of 2 B rows as well)
        }
        launch_splice_f32(m->row_src.as<int>(), (int)(B * S), m->embed, m->s_feats.as<float>(), m->x.as<float>(), c.hidden,
                          m->st, lo_plane(m, m->embed));
    } else {
        launch_splice(m->row_src.as<int>(), (int)(B * S), m->embed, m->feats.as<bf16_t>(), m->x.as<float>(), c.hidden, m->st);
    }
    HIPCHK(hipStreamSynchronize(m->st));  // `flat` is host memory
    m->curB = B;
    m->curS = (int)S;
    if (S_out) *S_out = (int)S;
}

// ---- token scores (vc_request_token_scores): log p(label) of the labelled positions, without logits leaving the device ------------
// Shift rule of [HF] LlamaForCausalLM.forward / the reference (vcoder_ds_llava_llama.py:95-106): labels[..., 1:] against
// logits[..., :-1, :] — the row in front of position j scores label j, position 0 is never scored.
// The rows of one launch sequence: the logits workspace is SCORE_CHUNK_ROWS x V floats however many rows carry a label
// (131 MB at V = 32000).
constexpr int SCORE_CHUNK_ROWS = 1024;
// log p(tgt[i]) from residual row row_idx[i] of x [., D]: per chunk the final RMSNorm gathered by row index, the lm_head over the
// chunk only, token_logprob_kernel over its logits — in the session's precision mode.  A bf16-mode chunk of up to SCORE_GEMV_ROWS rows
// takes ONE pass of the packed lm_head's GEMV as last_row_logits does, more rows the GEMM: at the lm_head's shape (N 32000, K 4096)
// every further GEMV pass streams the 262 MB weight again (+45 us) while the GEMM stays near 105 us up to 160 rows, so the
// layer linears' EXTEND_GEMV_ROWS = 128 does not hold here (tools/kbench.py score_head, DESIGN.md 4.4c: 16 rows 68 | 102 us,
// 32 rows 75 | 106, 64 rows 122 | 106, 128 rows 212 | 108).  The results land in m->sc_lp [row_idx.size()] on the device, in order;
// nothing is synchronised.
constexpr int SCORE_GEMV_ROWS = VC_GEMV_MAX_M;
// vc_request_top_logprobs: the stk_k most likely tokens of `nr` logits rows into rows [r0, r0 + nr) of m->sc_tlp / m->sc_tid (sized by
// ensure_score_top); nothing without the request
void ensure_score_top(vc_model* m, size_t rows) {
    if (!m->stk_k) return;
    m->sc_tlp.ensure(rows * m->stk_k * 4);
    m->sc_tid.ensure(rows * m->stk_k * 4);
}
void score_top_rows(vc_model* m, const float* logits, size_t r0, int nr) {
    if (!m->stk_k) return;
    const int K = m->stk_k, V = m->c.vocab;
    TopkLogprobArgs a{logits, V, nullptr, nullptr, m->sc_tlp.as<float>() + r0 * K, m->sc_tid.as<int>() + r0 * K, V, K, nullptr, nullptr, 0};
    launch_topk_logprob(a, nr, -1, m->st);
}
// the caller's top buffers: 0.0 / -1 over `positions` positions; then (top_scatter) device row i -> position pos of the call's layout
void top_fill(vc_model* m, size_t positions) {
    if (!m->stk_k) return;
    std::fill(m->stk_lp, m->stk_lp + positions * m->stk_k, 0.f);
    std::fill(m->stk_ids, m->stk_ids + positions * m->stk_k, -1);
}
struct TopHost {   // the device rows of a call on the host (one copy; the caller synchronises the stream before reading)
    std::vector<float> lp;
    std::vector<int32_t> id;
    int K = 0;
    void fetch(vc_model* m, size_t rows) {
        K = m->stk_k;
        if (!K || !rows) return;
        lp.resize(rows * K);
        id.resize(rows * K);
        HIPCHK(hipMemcpyAsync(lp.data(), m->sc_tlp.p, lp.size() * 4, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipMemcpyAsync(id.data(), m->sc_tid.p, id.size() * 4, hipMemcpyDeviceToHost, m->st));
    }
    void scatter(vc_model* m, size_t row, size_t pos) const {
        if (!K) return;
        std::copy(lp.begin() + row * K, lp.begin() + (row + 1) * K, m->stk_lp + pos * K);
        std::copy(id.begin() + row * K, id.begin() + (row + 1) * K, m->stk_ids + pos * K);
    }
};
void score_rows(vc_model* m, const float* x, const std::vector<int>& row_idx, const std::vector<int>& tgt) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, V = c.vocab, n = (int)row_idx.size();
    if (n == 0) return;
    const int chunk_cap = (int)rup(std::min(n, SCORE_CHUNK_ROWS), 32);   // (a GEMV pass holds 32 token slots)
    const int ldx = split_ld(D);
    m->sc_idx.ensure((size_t)2 * n * 4);
    m->sc_lp.ensure((size_t)n * 4);
    ensure_score_top(m, (size_t)n);
    m->sc_xn.ensure((size_t)chunk_cap * std::max((size_t)D * 4, (size_t)ldx * 2), true);
    m->sc_logits.ensure((size_t)chunk_cap * V * 4, true);
    int* idx_dev = m->sc_idx.as<int>();
    int* tgt_dev = idx_dev + n;
    HIPCHK(hipMemcpyAsync(idx_dev, row_idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(tgt_dev, tgt.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->st));
    float* lg = m->sc_logits.as<float>();
    for (int r0 = 0; r0 < n; r0 += SCORE_CHUNK_ROWS) {
        const int nr = std::min(SCORE_CHUNK_ROWS, n - r0);
        if (m->precision == 1) {
            launch_rmsnorm_f32(x, idx_dev + r0, m->final_norm, m->sc_xn.as<float>(), nr, D, c.rms_eps, m->st);
            gemm32(m, m->sc_xn.as<float>(), m->lm_head, nullptr, lg, nr, V, D, D, D, V, EPI_F32);
        } else if (m->precision == 2) {
            launch_rmsnorm_split(x, idx_dev + r0, m->final_norm, m->sc_xn.as<bf16_t>(), nr, D, c.rms_eps, ldx, D, m->st);
            gemm_split(m, m->sc_xn.as<bf16_t>(), m->lm_head, nullptr, lg, nr, V, D, V, EPI_F32, ldx);
        } else {
            launch_rmsnorm_rows(x, idx_dev + r0, m->final_norm, m->sc_xn.as<bf16_t>(), nr, D, c.rms_eps, m->st);
            if (nr <= SCORE_GEMV_ROWS) {
                LoopView lv{};   // the lm_head GEMV needs a stream only
                lv.st = m->st;
                gemv(m, lv, m->sc_xn.as<bf16_t>(), m->lm_head_p, nullptr, lg, nr, V, D, V, GEMV_F32);
            } else {
                gemm(m, m->sc_xn.as<bf16_t>(), m->lm_head, nullptr, lg, nr, V, D, V, EPI_F32);
            }
        }
        launch_token_logprob(lg, V, tgt_dev + r0, m->sc_lp.as<float>() + r0, nr, V, m->st);
        score_top_rows(m, lg, r0, nr);
    }
}
// the labelled positions of `labels` [B, n] (n rows per sequence in x): row b n + j - 1 scores label j >= 1.  The caller's buffer
// receives [B, n] floats, 0 where nothing is scored.  One device-to-host copy of the scored entries; synchronises the stream.
void score_labelled_rows(vc_model* m, const float* x, const int64_t* labels, int B, int n, float* out) {
    std::vector<int> row_idx, tgt;
    for (int b = 0; b < B; ++b)
        for (int j = 1; j < n; ++j) {
            const int64_t l = labels[(size_t)b * n + j];
            if (l == IGNORE_INDEX) continue;
            REQUIRE(l >= 0 && l < m->c.vocab, VC_ERR_INDEX, "Target %lld is out of bounds.", (long long)l);
            row_idx.push_back(b * n + j - 1);
            tgt.push_back((int)l);
        }
    std::fill(out, out + (size_t)B * n, 0.f);
    top_fill(m, (size_t)B * n);
    if (row_idx.empty()) return;
    score_rows(m, x, row_idx, tgt);
    std::vector<float> lp(row_idx.size());
    TopHost top;
    HIPCHK(hipMemcpyAsync(lp.data(), m->sc_lp.p, lp.size() * 4, hipMemcpyDeviceToHost, m->st));
    top.fetch(m, row_idx.size());
    HIPCHK(hipStreamSynchronize(m->st));
    for (size_t i = 0; i < lp.size(); ++i) {
        out[row_idx[i] + 1] = lp[i];
        top.scatter(m, i, (size_t)row_idx[i] + 1);
    }
}
// logits rows [B * n, V] already on the device (a continuation whose lm_head ran over every row): every row is scored in place —
// row b n + j - 1 against label j, unlabelled rows against token 0 and dropped on the host
void score_logits_rows(vc_model* m, const float* logits, const int64_t* labels, int B, int n, float* out) {
    const int M = B * n;
    std::vector<int> tgt(M, 0);
    bool any = false;
    for (int b = 0; b < B; ++b)
        for (int j = 1; j < n; ++j) {
            const int64_t l = labels[(size_t)b * n + j];
            if (l == IGNORE_INDEX) continue;
            tgt[b * n + j - 1] = (int)l;
            any = true;
        }
    std::fill(out, out + (size_t)M, 0.f);
    top_fill(m, (size_t)M);
    if (!any) return;
    m->sc_idx.ensure((size_t)M * 4);
    m->sc_lp.ensure((size_t)M * 4);
    ensure_score_top(m, (size_t)M);
    HIPCHK(hipMemcpyAsync(m->sc_idx.p, tgt.data(), (size_t)M * 4, hipMemcpyHostToDevice, m->st));
    launch_token_logprob(logits, m->c.vocab, m->sc_idx.as<int>(), m->sc_lp.as<float>(), M, m->c.vocab, m->st);
    score_top_rows(m, logits, 0, M);
    std::vector<float> lp(M);
    TopHost top;
    HIPCHK(hipMemcpyAsync(lp.data(), m->sc_lp.p, (size_t)M * 4, hipMemcpyDeviceToHost, m->st));
    top.fetch(m, (size_t)M);
    HIPCHK(hipStreamSynchronize(m->st));
    for (int b = 0; b < B; ++b)
        for (int j = 1; j < n; ++j)
            if (labels[(size_t)b * n + j] != IGNORE_INDEX) {
                out[b * n + j] = lp[b * n + j - 1];
                top.scatter(m, (size_t)b * n + j - 1, (size_t)b * n + j);
            }
}

// decoder stack over the spliced batch + last-row logits (m->logits [B,V]); keys / values go to `kv`
void finish_prefill(vc_model* m, const KvTarget& kv, float* logits_all_host) {
    const vc_model_cfg& c = m->c;
    const int B = m->curB, S = m->curS, D = c.hidden;
    std::vector<int> idx(B);   // strict / split: the last row of every sequence
    for (int b = 0; b < B; ++b) idx[b] = b * S + S - 1;
    if (m->precision) HIPCHK(hipMemcpyAsync(m->last_idx.p, idx.data(), B * 4, hipMemcpyHostToDevice, m->st));
    emit_hidden(m, 0, B, S);   // inputs_embeds
    if (m->precision == 1) {
        run_llm_layers_strict(m, m->x.as<float>(), B, S, nullptr, true, kv.row0);
        logits_strict(m, m->x.as<float>(), m->last_idx.as<int>(), B);
    } else if (m->precision == 2) {
        run_prefill_layers_split(m, kv, B, S);
        // final norm of the last rows as one stacked hi / lo group of the split GEMV, then lm_head
        const int G = B <= 8 ? 8 : 16;
        m->xl.ensure((size_t)2 * 16 * D * 2, true);
        launch_rmsnorm_split(m->x.as<float>(), m->last_idx.as<int>(), m->final_norm, m->xl.as<bf16_t>(), B, D, c.rms_eps, D,
                             (size_t)G * D, m->st);
        LoopView lv{};
        lv.st = m->st;
        lv.split_G = G;
        gemv(m, lv, m->xl.as<bf16_t>(), m->lm_head_p, nullptr, m->logits.p, B, c.vocab, D, c.vocab, GEMV_F32);
    } else {
        run_prefill_layers(m, kv, B, S);
        last_row_logits(m, m->x.as<float>(), B, S);
    }
    if (logits_all_host) {  // lm_head over ALL S positions, as the reference's forward returns (:93)
        const size_t Mr = (size_t)B * S;
        m->logits_all.ensure(Mr * c.vocab * 4);
        if (m->precision == 1) {
            launch_rmsnorm_f32(m->x.as<float>(), nullptr, m->final_norm, m->s_xn.as<float>(), (int)Mr, D, c.rms_eps, m->st);
            gemm32(m, m->s_xn.as<float>(), m->lm_head, nullptr, m->logits_all.as<float>(), (int)Mr, c.vocab, D, D, D, c.vocab,
                   EPI_F32);
        } else if (m->precision == 2) {
            const int ldx = split_ld(D);
            m->xn.ensure(Mr * ldx * 2);
            launch_rmsnorm_split(m->x.as<float>(), nullptr, m->final_norm, m->xn.as<bf16_t>(), (int)Mr, D, c.rms_eps, ldx, D, m->st);
            gemm_split(m, m->xn.as<bf16_t>(), m->lm_head, nullptr, m->logits_all.p, (int)Mr, c.vocab, D, c.vocab, EPI_F32, ldx);
        } else {
            all_row_logits(m, m->x.as<float>(), (int)Mr);
        }
        HIPCHK(hipMemcpyAsync(logits_all_host, m->logits_all.p, Mr * c.vocab * 4, hipMemcpyDeviceToHost, m->st));
    }
    if (m->score_on) {   // vc_request_token_scores: the labelled rows only, whatever else was asked for
        score_labelled_rows(m, m->x.as<float>(), m->spliced_labels.data(), B, S, m->score_out);
        if (m->score_labels_out) std::copy(m->spliced_labels.begin(), m->spliced_labels.end(), m->score_labels_out);
    }
    HIPCHK(hipStreamSynchronize(m->st));  // `idx` is host memory
    m->hidden_out = nullptr;               // one-shot
    m->attn_out = nullptr;
}

// arm the session's own loop for the B rows just prefilled (fan > 1: the B x fan rows that continue them): every row at position S,
// step 0
void arm_session_rows(vc_model* m, const GenParams& g, const int* tail, int fan = 1) {
    const int B = m->curB * fan, S = m->curS;
    std::vector<int> rec((size_t)B * RS_STRIDE);
    fill_rows(rec.data(), B, g, S, tail, 0, m->out_stride, fan);
    HIPCHK(hipMemsetAsync(m->rows.p, 0, m->rows.cap, m->st));
    HIPCHK(hipMemcpyAsync(m->rows.p, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    m->cur_pos = S;
    m->spec_closed = false;
    m->fan_closed = false;
    m->gd_closed = false;
    m->tok_stale = false;
}

// arm the session's loop for a guided call (vc_request_guidance): rows 0 .. B - 1 continue the B prompts at position S_c with the
// call's parameters and the scale; rows B .. 2 B - 1 are their followers at position S_n — active, nothing recorded (RS_MAXNEW 0),
// no EOS or stop sequence of their own (guidance_follow_kernel mirrors RS_FINISHED)
void arm_guided_rows(vc_model* m, const GenParams& g, const int* tail, int B, int S_c, int S_n, float scale) {
    std::vector<int> rec((size_t)2 * B * RS_STRIDE);
    fill_rows(rec.data(), B, g, S_c, tail, 0, m->out_stride);
    GenParams f;
    f.pad = g.pad;
    fill_rows(rec.data() + (size_t)B * RS_STRIDE, B, f, S_n, nullptr, 0, 0);
    for (int b = 0; b < B; ++b) memcpy(&rec[(size_t)b * RS_STRIDE + RS_GD_SCALE], &scale, 4);
    HIPCHK(hipMemsetAsync(m->rows.p, 0, m->rows.cap, m->st));
    HIPCHK(hipMemcpyAsync(m->rows.p, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    m->cur_pos = std::max(S_c, S_n);
    m->spec_closed = false;
    m->fan_closed = false;
    m->gd_closed = false;
    m->tok_stale = false;
}

