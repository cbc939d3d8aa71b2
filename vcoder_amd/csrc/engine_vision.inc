// engine_vision.inc — part of the host engine (textually included by engine.hip inside its anonymous namespace; one translation unit).
// CLIP tower + adapters of the three precision modes (bf16, split, strict): encode_images / encode_seg_images / encode_depth_images.

// ------------------------------------------------------------------------------------------------
// ViT: pixels of all modalities batched into ONE tower pass (the tower weights are shared).  A modality may carry
// any number of images (the reference's list / 5-D image form gives a sample several images, vcoder_ds_llava_arch.py:
// 135-143); the common 4-D form has one image per sample and modality.
struct PixSet {
    const float* p[3];  // IMAGE, SEG, DEPTH pixel blocks (nullptr = modality absent)
    int n[3];           // images in each block
};

inline bool has_mod(const PixSet& in, int k) { return in.p[k] && in.n[k] > 0; }

// Pixel staging of a tower pass: counts the modalities present (`order`: their blocks in v_pixels, `first_img[k]`: the first
// image of modality k's block), sizes v_pixels for all N images and copies in the blocks of the modalities in `copy_mask`
// (bit k; the splice plan alone reads only the depth pixels).  Returns N.
int stage_pixels(vc_model* m, const PixSet& in, int pixels_on_device, int order[3], int first_img[3], unsigned copy_mask = 7) {
    int nmod = 0, N = 0;
    for (int k = 0; k < 3; ++k) {
        first_img[k] = 0;
        if (has_mod(in, k)) {
            order[nmod++] = k;
            first_img[k] = N;
            N += in.n[k];
        }
    }
    REQUIRE(N > 0, VC_ERR_INVALID, "no images");
    const size_t img_elems = (size_t)3 * m->c.vit_image * m->c.vit_image;
    m->v_pixels.ensure((size_t)N * img_elems * 4);
    for (int i = 0; i < nmod; ++i) {
        const int k = order[i];
        if (!(copy_mask >> k & 1)) continue;
        HIPCHK(hipMemcpyAsync(m->v_pixels.as<float>() + (size_t)first_img[k] * img_elems, in.p[k],
                              (size_t)in.n[k] * img_elems * 4,
                              pixels_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, m->st));
    }
    return N;
}

// what the splice planner reads of the features: modality k owns rows [feat_off, feat_off + feat_rows) of the feature buffer
// (R rows per image, blocks in the order of v_pixels)
void set_feat_rows(vc_model* m, const PixSet& in, const int first_img[3], int R) {
    for (int k = 0; k < 3; ++k) {
        m->feat_rows[k] = 0;
        if (!has_mod(in, k)) continue;
        m->feat_off[k] = first_img[k] * R;
        m->feat_rows[k] = in.n[k] * R;
    }
}

// The adapters behind the tower (encode_images / encode_seg_images / encode_depth_images, vcoder_ds_llava_arch.py:106-124),
// stated once for the three precision modes.  A mode describes its buffers (rows in bytes):
struct AdapterForm {
    const char* src;    // feature_select'ed tower rows
    size_t src_row;
    char* out;          // projected features (what the splice reads)
    size_t out_row;
    Buf *mid0, *mid1;   // outputs of the middle layers of a projector, alternating
    size_t mid_row;
};
// and supplies two callables: identity_rows() -> the rows a depth-0 projector copies (in the features' element type, all images),
// and linear(cur, l, W, b, dst, rows, last): layer l of a projector over `rows` rows (GELU unless last)
template <class IdentityRows, class Linear>
void run_adapters(vc_model* m, const PixSet& in, const int first_img[3], const AdapterForm& f, IdentityRows&& identity_rows,
                  Linear&& linear) {
    const int R = m->Tv - (m->c.vit_keep_cls ? 0 : 1);  // feature rows per image
    set_feat_rows(m, in, first_img, R);
    for (int mod = 0; mod < 3; ++mod) {
        if (!has_mod(in, mod)) continue;
        // images -> mm_projector; seg AND depth -> seg_mm_projector (quirk 1, vcoder_ds_llava_arch.py:111-114);
        // mm2_projector is unreachable (quirk 2, :137,145)
        const Projector& pj = mod == VC_MOD_IMAGE ? m->mm : m->seg;
        const int rows = m->feat_rows[mod];
        const size_t row0 = (size_t)m->feat_off[mod];
        char* out = f.out + row0 * f.out_row;
        if (pj.depth == 0) {
            REQUIRE(m->c.vit_hidden == m->c.hidden, VC_ERR_INVALID, "identity projector needs mm_hidden_size == hidden_size");
            HIPCHK(hipMemcpyAsync(out, identity_rows() + row0 * f.out_row, (size_t)rows * f.out_row, hipMemcpyDeviceToDevice, m->st));
            continue;
        }
        const void* cur = f.src + row0 * f.src_row;
        for (int l = 0; l < pj.depth; ++l) {
            const bool last = l == pj.depth - 1;
            void* dst = out;
            if (!last) {
                Buf* mid = l % 2 == 0 ? f.mid0 : f.mid1;
                mid->ensure((size_t)rows * f.mid_row);
                dst = mid->p;
            }
            linear(cur, l, pj.w[l], pj.b[l], dst, rows, last);
            cur = dst;
        }
    }
}

// CLIPVisionTower.forward (clip_encoder.py:39-51) up to hidden_states[select_layer]: leaves the fp32 residual stream of
// all N images in v_x [N*Tv, Dv]; returns N and the block order
int run_vit_tower(vc_model* m, const PixSet& in, int pixels_on_device, int order[3], int first_img[3]) {
    const vc_model_cfg& c = m->c;
    const int Dv = c.vit_hidden, Fv = c.vit_ffn, H = c.vit_heads, Tv = m->Tv, P = m->P;
    const int N = stage_pixels(m, in, pixels_on_device, order, first_img);
    const int M = N * Tv, Mp = N * P;
    const int Ts = (int)rup(Tv, 64);
    m->v_cols.ensure((size_t)Mp * m->Kpad * 2);
    m->v_patches.ensure((size_t)Mp * Dv * 4);
    m->v_x.ensure((size_t)M * Dv * 4);
    m->v_xn.ensure((size_t)M * Dv * 2);
    m->v_qkv.ensure((size_t)M * 3 * Dv * 2);
    m->v_q.ensure((size_t)N * H * Ts * m->vhd * 2, true);
    m->v_k.ensure((size_t)N * H * Ts * m->vhd * 2, true);
    m->v_vt.ensure((size_t)N * H * Ts * m->vhd * 2, true);
    m->v_attn.ensure((size_t)M * Dv * 2);
    m->v_h.ensure((size_t)M * Fv * 2);
    launch_im2col(m->v_pixels.as<float>(), m->v_cols.as<bf16_t>(), N, c.vit_image, c.vit_patch, m->Kpad, m->st);
    gemm(m, m->v_cols.as<bf16_t>(), m->vit_patch_w, nullptr, m->v_patches.p, Mp, Dv, m->Kpad, Dv, EPI_F32);
    launch_vit_embed_ln(m->v_patches.as<float>(), m->vit_cls, m->vit_pos, m->vit_pre_w, m->vit_pre_b, m->v_x.as<float>(),
                        N, Tv, Dv, c.vit_ln_eps, m->st);
    for (int j = 0; j < c.vit_layers_used; ++j) {
        const VitLayer& L = m->vit[j];
        launch_layernorm(m->v_x.as<float>(), L.ln1_w, L.ln1_b, m->v_xn.as<bf16_t>(), M, Dv, c.vit_ln_eps, m->st);
        gemm(m, m->v_xn.as<bf16_t>(), L.qkv_w, L.qkv_b, m->v_qkv.p, M, 3 * Dv, Dv, 3 * Dv, EPI_BF16);
        QkvSplitArgs qa{m->v_qkv.as<bf16_t>(), m->v_q.as<bf16_t>(), m->v_k.as<bf16_t>(), m->v_vt.as<bf16_t>(), N, Tv, H,
                        m->vhd, Ts, Ts, nullptr, nullptr, nullptr};
        launch_qkv_split(qa, m->st);
        AttnArgs aa{m->v_q.as<bf16_t>(), m->v_k.as<bf16_t>(), m->v_vt.as<bf16_t>(), m->v_attn.as<bf16_t>(), N, H, Tv,
                    m->vhd, Ts, Ts, 0, 1.0f / sqrtf((float)m->vhd)};
        launch_attention(aa, m->st);
        gemm(m, m->v_attn.as<bf16_t>(), L.out_w, L.out_b, m->v_x.p, M, Dv, Dv, Dv, EPI_RESID_F32);
        launch_layernorm(m->v_x.as<float>(), L.ln2_w, L.ln2_b, m->v_xn.as<bf16_t>(), M, Dv, c.vit_ln_eps, m->st);
        gemm(m, m->v_xn.as<bf16_t>(), L.fc1_w, L.fc1_b, m->v_h.p, M, Fv, Dv, Fv, EPI_BF16_QGELU);
        gemm(m, m->v_h.as<bf16_t>(), L.fc2_w, L.fc2_b, m->v_x.p, M, Dv, Fv, Dv, EPI_RESID_F32);
    }
    // feature_select (clip_encoder.py:29-37): hidden_states[select_layer] is the last layer evaluated; drop CLS for 'patch'
    const int skip = c.vit_keep_cls ? 0 : 1;
    const int R = Tv - skip;
    m->v_sel.ensure((size_t)N * R * Dv * 2);
    launch_select_rows_bf16(m->v_x.as<float>(), m->v_sel.as<bf16_t>(), N, Tv, skip, Dv, m->st);
    return N;
}

void run_vit_and_adapters(vc_model* m, const PixSet& in, int pixels_on_device) {
    const int Dv = m->c.vit_hidden, D = m->c.hidden;
    int order[3], first_img[3];
    const int N = run_vit_tower(m, in, pixels_on_device, order, first_img);
    const int R = m->Tv - (m->c.vit_keep_cls ? 0 : 1);  // feature rows per image
    m->feats.ensure((size_t)N * R * D * 2);
    m->v_mid.ensure((size_t)N * R * D * 2);
    const AdapterForm f{m->v_sel.as<char>(), (size_t)Dv * 2, m->feats.as<char>(), (size_t)D * 2, &m->v_mid, &m->v_h, (size_t)D * 2};
    run_adapters(m, in, first_img, f, [&] { return f.src; },
                 [&](const void* cur, int l, const bf16_t* W, const float* b, void* dst, int rows, bool last) {
                     gemm(m, static_cast<const bf16_t*>(cur), W, b, dst, rows, D, l ? D : Dv, D, last ? EPI_BF16 : EPI_BF16_GELU);
                 });
}

// ------------------------------------------------------------------------------------------------
// SPLIT path (precision 2): the fast path's kernels and sequence of operations with every MFMA operand carried as bf16
// hi + lo (x = hi + lo to ~16 mantissa bits; weights are exactly bf16): GEMMs contract the [hi | lo] rows against the weight
// twice, attention uses three MFMAs per product, and everything between two MFMAs stays fp32.  Leaves the fp32 residual
// stream of all N images in v_x [N*Tv, Dv].
int run_vit_tower_split(vc_model* m, const PixSet& in, int pixels_on_device, int order[3], int first_img[3]) {
    const vc_model_cfg& c = m->c;
    const int Dv = c.vit_hidden, Fv = c.vit_ffn, H = c.vit_heads, Tv = m->Tv, P = m->P;
    const int N = stage_pixels(m, in, pixels_on_device, order, first_img);
    const int M = N * Tv, Mp = N * P;
    const int Ts = (int)rup(Tv, 64);
    const int ldx = split_ld(Dv), ldh = split_ld(Fv);
    m->v_cols.ensure((size_t)Mp * 2 * m->Kpad * 2);
    m->v_patches.ensure((size_t)Mp * Dv * 4);
    m->v_x.ensure((size_t)M * Dv * 4);
    m->v_xn.ensure((size_t)M * ldx * 2);
    m->s_vqkv.ensure((size_t)M * 3 * Dv * 4);
    const size_t plane = (size_t)N * H * Ts * m->vhd;   // one bf16 plane of Q / K / V^T
    m->v_q.ensure(2 * plane * 2, true);
    m->v_k.ensure(2 * plane * 2, true);
    m->v_vt.ensure(2 * plane * 2, true);
    m->v_attn.ensure((size_t)M * ldx * 2);
    m->v_h.ensure((size_t)M * ldh * 2);
    launch_im2col(m->v_pixels.as<float>(), m->v_cols.as<bf16_t>(), N, c.vit_image, c.vit_patch, m->Kpad, m->st, true);
    gemm_split(m, m->v_cols.as<bf16_t>(), m->vit_patch_w, nullptr, m->v_patches.p, Mp, Dv, m->Kpad, Dv, EPI_F32, 2 * m->Kpad);
    launch_vit_embed_ln(m->v_patches.as<float>(), m->vit_cls, m->vit_pos, m->vit_pre_w, m->vit_pre_b, m->v_x.as<float>(),
                        N, Tv, Dv, c.vit_ln_eps, m->st);
    bf16_t *qh = m->v_q.as<bf16_t>(), *kh = m->v_k.as<bf16_t>(), *vh = m->v_vt.as<bf16_t>();
    for (int j = 0; j < c.vit_layers_used; ++j) {
        const VitLayer& L = m->vit[j];
        launch_layernorm_split(m->v_x.as<float>(), L.ln1_w, L.ln1_b, m->v_xn.as<bf16_t>(), M, Dv, c.vit_ln_eps, ldx, Dv, m->st);
        gemm_split(m, m->v_xn.as<bf16_t>(), L.qkv_w, L.qkv_b, m->s_vqkv.p, M, 3 * Dv, Dv, 3 * Dv, EPI_F32, ldx);
        QkvSplit32Args qa{m->s_vqkv.as<float>(), qh, qh + plane, kh, kh + plane, vh, vh + plane, nullptr, nullptr,
                          N, Tv, H, m->vhd, Ts, Ts, Ts, 0, nullptr, nullptr};
        launch_qkv_split32(qa, m->st);
        AttnArgs aa{qh, kh, vh, m->v_attn.as<bf16_t>(), N, H, Tv, m->vhd, Ts, Ts, 0, 1.0f / sqrtf((float)m->vhd), 0,
                    qh + plane, kh + plane, vh + plane, ldx, Dv};
        launch_attention(aa, m->st);
        gemm_split(m, m->v_attn.as<bf16_t>(), L.out_w, L.out_b, m->v_x.p, M, Dv, Dv, Dv, EPI_RESID_F32, ldx);
        launch_layernorm_split(m->v_x.as<float>(), L.ln2_w, L.ln2_b, m->v_xn.as<bf16_t>(), M, Dv, c.vit_ln_eps, ldx, Dv, m->st);
        gemm_split(m, m->v_xn.as<bf16_t>(), L.fc1_w, L.fc1_b, m->v_h.p, M, Fv, Dv, ldh, EPI_BF16_QGELU, ldx, Fv);
        gemm_split(m, m->v_h.as<bf16_t>(), L.fc2_w, L.fc2_b, m->v_x.p, M, Dv, Fv, Dv, EPI_RESID_F32, ldh);
    }
    return N;
}

// feature_select + adapters of the split path: projected features fp32 in s_feats (what the fp32 splice reads)
void run_vit_and_adapters_split(vc_model* m, const PixSet& in, int pixels_on_device) {
    const vc_model_cfg& c = m->c;
    const int Dv = c.vit_hidden, D = c.hidden;
    int order[3], first_img[3];
    const int N = run_vit_tower_split(m, in, pixels_on_device, order, first_img);
    const int skip = c.vit_keep_cls ? 0 : 1;
    const int R = m->Tv - skip;  // feature rows per image
    const int ldv = 2 * Dv, ldd = split_ld(D);
    m->v_sel.ensure((size_t)N * R * ldv * 2);
    launch_select_rows_bf16(m->v_x.as<float>(), m->v_sel.as<bf16_t>(), N, m->Tv, skip, Dv, m->st, true);
    m->s_feats.ensure((size_t)N * R * D * 4);
    m->v_mid.ensure((size_t)N * R * ldd * 2);
    const AdapterForm f{m->v_sel.as<char>(), (size_t)ldv * 2, m->s_feats.as<char>(), (size_t)D * 4, &m->v_mid, &m->v_h, (size_t)ldd * 2};
    run_adapters(
        m, in, first_img, f,
        [&] {  // identity: the fp32 rows of hidden_states[select_layer]
            m->s_sel.ensure((size_t)N * R * Dv * 4);
            launch_select_rows_f32(m->v_x.as<float>(), m->s_sel.as<float>(), N, m->Tv, skip, Dv, m->st);
            return m->s_sel.as<char>();
        },
        [&](const void* cur, int l, const bf16_t* W, const float* b, void* dst, int rows, bool last) {
            const bf16_t* A = static_cast<const bf16_t*>(cur);
            const int K = l ? D : Dv, lda = l ? ldd : ldv;
            if (last) gemm_split(m, A, W, b, dst, rows, D, K, D, EPI_F32, lda);
            else gemm_split(m, A, W, b, dst, rows, D, K, ldd, EPI_BF16_GELU, lda, D);
        });
}

// ------------------------------------------------------------------------------------------------
// STRICT (fp32-faithful) path: same sequence of operations, fp32 activations, strict.hip kernels, no graph.
void gemm32(vc_model* m, const float* A, const bf16_t* W, const float* bias, float* out, int M, int N, int K, int lda,
            int ldw, int ldo, int epi) {
    GemmF32Args a{A, W, bias, out, M, N, K, lda, ldw, ldo};
    a.W_lo = lo_plane(m, W);
    launch_gemm_f32(a, epi, m->st);
}

int run_vit_tower_strict(vc_model* m, const PixSet& in, int pixels_on_device, int order[3], int first_img[3]) {
    const vc_model_cfg& c = m->c;
    const int Dv = c.vit_hidden, Fv = c.vit_ffn, H = c.vit_heads, Tv = m->Tv, P = m->P, D = c.hidden;
    const int N = stage_pixels(m, in, pixels_on_device, order, first_img);
    const int M = N * Tv, Mp = N * P;
    m->s_cols.ensure((size_t)Mp * m->Kpatch * 4);
    m->s_patches.ensure((size_t)Mp * Dv * 4);
    m->s_vx.ensure((size_t)M * Dv * 4);
    m->s_vxn.ensure((size_t)M * Dv * 4);
    m->s_vqkv.ensure((size_t)M * 3 * Dv * 4);
    m->s_vq.ensure((size_t)M * Dv * 4);
    m->s_vk.ensure((size_t)M * Dv * 4);
    m->s_vv.ensure((size_t)M * Dv * 4);
    m->s_vattn.ensure((size_t)M * Dv * 4);
    m->s_vh.ensure((size_t)M * std::max(Fv, D) * 4);
    float *x = m->s_vx.as<float>(), *xn = m->s_vxn.as<float>();
    launch_im2col_f32(m->v_pixels.as<float>(), m->s_cols.as<float>(), N, c.vit_image, c.vit_patch, m->st);
    gemm32(m, m->s_cols.as<float>(), m->vit_patch_w, nullptr, m->s_patches.as<float>(), Mp, Dv, m->Kpatch, m->Kpatch, m->Kpad,
           Dv, EPI_F32);
    launch_vit_embed_ln(m->s_patches.as<float>(), m->vit_cls, m->vit_pos, m->vit_pre_w, m->vit_pre_b, x, N, Tv, Dv,
                        c.vit_ln_eps, m->st);
    for (int j = 0; j < c.vit_layers_used; ++j) {
        const VitLayer& L = m->vit[j];
        launch_layernorm_f32(x, L.ln1_w, L.ln1_b, xn, M, Dv, c.vit_ln_eps, m->st);
        gemm32(m, xn, L.qkv_w, L.qkv_b, m->s_vqkv.as<float>(), M, 3 * Dv, Dv, Dv, Dv, 3 * Dv, EPI_F32);
        QkvF32Args qa{m->s_vqkv.as<float>(), m->s_vq.as<float>(), m->s_vk.as<float>(), m->s_vv.as<float>(), N, Tv, H, m->vhd,
                      Tv, Tv, nullptr, nullptr, nullptr};
        launch_qkv_rope_f32(qa, m->st);
        AttnF32Args aa{m->s_vq.as<float>(), m->s_vk.as<float>(), m->s_vv.as<float>(), m->s_vattn.as<float>(), N, H, Tv, m->vhd,
                       Tv, Tv, 0, Tv, nullptr, 1.0f / sqrtf((float)m->vhd)};
        launch_attention_f32(aa, m->st);
        gemm32(m, m->s_vattn.as<float>(), L.out_w, L.out_b, x, M, Dv, Dv, Dv, Dv, Dv, EPI_RESID_F32);
        launch_layernorm_f32(x, L.ln2_w, L.ln2_b, xn, M, Dv, c.vit_ln_eps, m->st);
        gemm32(m, xn, L.fc1_w, L.fc1_b, m->s_vh.as<float>(), M, Fv, Dv, Dv, Dv, Fv, EPI_BF16_QGELU);
        gemm32(m, m->s_vh.as<float>(), L.fc2_w, L.fc2_b, x, M, Dv, Fv, Fv, Fv, Dv, EPI_RESID_F32);
    }
    const int skip = c.vit_keep_cls ? 0 : 1;
    const int R = Tv - skip;
    m->s_sel.ensure((size_t)N * R * Dv * 4);
    launch_select_rows_f32(x, m->s_sel.as<float>(), N, Tv, skip, Dv, m->st);
    return N;
}

void run_vit_and_adapters_strict(vc_model* m, const PixSet& in, int pixels_on_device) {
    const vc_model_cfg& c = m->c;
    const int Dv = c.vit_hidden, D = c.hidden;
    int order[3], first_img[3];
    const int N = run_vit_tower_strict(m, in, pixels_on_device, order, first_img);
    const int R = m->Tv - (c.vit_keep_cls ? 0 : 1);
    m->s_feats.ensure((size_t)N * R * D * 4);
    m->s_mid.ensure((size_t)N * R * D * 4);
    // (s_vh, the tower's MLP buffer, already holds N * Tv rows of max(vit_ffn, hidden) floats)
    const AdapterForm f{m->s_sel.as<char>(), (size_t)Dv * 4, m->s_feats.as<char>(), (size_t)D * 4, &m->s_mid, &m->s_vh, (size_t)D * 4};
    run_adapters(m, in, first_img, f, [&] { return f.src; },
                 [&](const void* cur, int l, const bf16_t* W, const float* b, void* dst, int rows, bool last) {
                     const int K = l ? D : Dv;
                     gemm32(m, static_cast<const float*>(cur), W, b, static_cast<float*>(dst), rows, D, K, K, K, D,
                            last ? EPI_F32 : EPI_BF16_GELU);
                 });
}

void ensure_strict(vc_model* m, int B, int Scap) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn, H = c.heads;
    if (B != m->s_capB || Scap > m->s_capS) {
        const size_t per_layer = (size_t)B * H * Scap * m->hd;
        m->s_kc.release();
        m->s_vc.release();
        m->s_kc.ensure(per_layer * c.layers * 4, true);
        m->s_vc.ensure(per_layer * c.layers * 4, true);
        m->s_capB = B;
        m->s_capS = Scap;
    }
    const size_t Mr = (size_t)B * Scap;
    m->s_xn.ensure(Mr * D * 4);
    m->s_qkv.ensure(Mr * 3 * D * 4);
    m->s_q.ensure(Mr * D * 4);
    m->s_attn.ensure(Mr * D * 4);
    m->s_h.ensure(Mr * F * 4);
    m->s_xl.ensure((size_t)rup(B, 16) * D * 4);
}
float* s_kcache(vc_model* m, int l) { return m->s_kc.as<float>() + (size_t)l * m->s_capB * m->c.heads * m->s_capS * m->hd; }
float* s_vcache(vc_model* m, int l) { return m->s_vc.as<float>() + (size_t)l * m->s_capB * m->c.heads * m->s_capS * m->hd; }

// one decoder stack pass over `T` new tokens per sample starting at the device-scalar position (prefill: pos 0).
// is_prefill says which of the two the pass is — a text-only prefill of ONE token has T == 1 too
// row0: the B sequences are cache rows row0 .. row0 + B - 1 (a guided prefill's negative prompts); pos_stride != 0: sequence b
// stands at pos_dev[b * pos_stride] (the rows' RS_POS: the pairs of a guided loop stand at different positions)
void run_llm_layers_strict(vc_model* m, float* x, int B, int T, const int* pos_dev, bool is_prefill, int row0 = 0, int pos_stride = 0) {
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn, H = c.heads, M = B * T;
    float *xn = m->s_xn.as<float>(), *qkv = m->s_qkv.as<float>(), *q = m->s_q.as<float>(), *at = m->s_attn.as<float>(),
          *h = m->s_h.as<float>();
    const int nl = (m->layer_limit > 0 && is_prefill) ? std::min(m->layer_limit, c.layers) : c.layers;
    for (int l = 0; l < nl; ++l) {
        const LlmLayer& L = m->llm[l];
        launch_rmsnorm_f32(x, nullptr, L.in_norm, xn, M, D, c.rms_eps, m->st);
        gemm32(m, xn, L.qkv_w, nullptr, qkv, M, 3 * D, D, D, D, 3 * D, EPI_F32);
        const size_t roff = (size_t)row0 * H * m->s_capS * m->hd;
        float *kl = s_kcache(m, l) + roff, *vl = s_vcache(m, l) + roff;
        QkvF32Args qa{qkv, q, kl, vl, B, T, H, m->hd, T, m->s_capS, pos_dev, m->rope_cos, m->rope_sin, pos_stride};
        launch_qkv_rope_f32(qa, m->st);
        AttnF32Args aa{q, kl, vl, at, B, H, T, m->hd, T, m->s_capS, 1, 0, pos_dev, 1.0f / sqrtf((float)m->hd)};
        aa.pos_stride = pos_stride;
        attach_kmask(m, aa, is_prefill ? m->has_kmask : m->kmask_in_decode);
        launch_attention_f32(aa, m->st);
        const bool step = !is_prefill && x == m->x_dec.as<float>();   // a session's cached decode step (m->cur_pos = its position)
        const bool pre = is_prefill && x == m->x.as<float>();
        if (pre || step) {
            AttnProbsArgs pa{};
            pa.q32 = q;
            pa.k32 = s_kcache(m, l);
            pa.q_stride = T;
            pa.kv_stride = m->s_capS;
            if (step) emit_attentions(m, l, B, 1, pa, m->cur_pos + 1, m->cur_pos);
            else emit_attentions(m, l, B, T, pa);
        }
        gemm32(m, at, L.o_w, nullptr, x, M, D, D, D, D, D, EPI_RESID_F32);
        launch_rmsnorm_f32(x, nullptr, L.post_norm, xn, M, D, c.rms_eps, m->st);
        gemm32(m, xn, L.gu_w, nullptr, h, M, 2 * F, D, D, D, F, EPI_SWIGLU);
        gemm32(m, h, L.down_w, nullptr, x, M, D, F, F, F, D, EPI_RESID_F32);
        if (pre) emit_hidden(m, l + 1, B, T);
        else if (step) emit_hidden(m, l + 1, B, 1, x);
    }
}

void logits_strict(vc_model* m, const float* x, const int* row_idx, int rows) {
    launch_rmsnorm_f32(x, row_idx, m->final_norm, m->s_xl.as<float>(), rows, m->c.hidden, m->c.rms_eps, m->st);
    gemm32(m, m->s_xl.as<float>(), m->lm_head, nullptr, m->logits.as<float>(), rows, m->c.vocab, m->c.hidden, m->c.hidden,
           m->c.hidden, m->c.vocab, EPI_F32);
}

