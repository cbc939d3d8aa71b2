// engine_profile.inc — part of the host engine (textually included by engine.hip): device preprocessing entry point, timings, the
// profile hooks bench.py uses (decode attention / GEMV replays, in-situ pool stamps) and the pool's policy setters.

namespace {
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
// bounds[2*o] = first tap, bounds[2*o+1] = tap count; kk[o*ksize + t] = fixed-point weight
int resample_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk) {
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale, ss = 1.0 / fs;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int n = xmax - xmin;
        double tot = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = bicubic_filter((x + xmin - center + 0.5) * ss);
            tot += w[x];
        }
        for (int x = 0; x < n; ++x) {
            const double v = tot != 0.0 ? w[x] / tot : w[x];
            kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << 22)) : (int)(0.5 + v * (double)(1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
    return ksize;
}
}  // namespace

/* One image: uint8 RGB [h,w,3] (host) -> fp32 [3,S,S] CLIP-normalised pixels (device when out_on_device, else host).
 * pad_to_square = the reference's image_aspect_ratio == 'pad' path (mm_utils.py:31-35): expand2square with the mean
 * colour, then resize to S x S; otherwise resize the shortest edge to S (bicubic) and center-crop S x S. */
VC_API int vc_preprocess_image(vc_model* m, const uint8_t* rgb, int h, int w, int pad_to_square, const float* mean,
                               const float* stdv, float* out, int out_on_device) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(rgb && out && mean && stdv && h > 0 && w > 0, VC_ERR_INVALID, "bad preprocess arguments");
    const int S = m->c.vit_image;
    m->pp_src.ensure((size_t)h * w * 3);
    HIPCHK(hipMemcpyAsync(m->pp_src.p, rgb, (size_t)h * w * 3, hipMemcpyHostToDevice, m->st));
    const uint8_t* cur = m->pp_src.as<uint8_t>();
    int ch = h, cw = w;
    if (pad_to_square && h != w) {
        const int side = h > w ? h : w;
        const int fill[3] = {(int)(mean[0] * 255), (int)(mean[1] * 255), (int)(mean[2] * 255)};  // int(x*255), mm_utils.py:33
        m->pp_sq.ensure((size_t)side * side * 3);
        launch_pad_square(cur, h, w, m->pp_sq.as<uint8_t>(), side, (side - w) / 2, (side - h) / 2, fill, m->st);
        cur = m->pp_sq.as<uint8_t>();
        ch = cw = side;
    }
    // shortest edge -> S, long edge = int(S * long / short)   ([HF] get_resize_output_image_size, default_to_square=False)
    int nh, nw;
    if (ch <= cw) { nh = S; nw = (int)((double)S * cw / ch); }
    else { nw = S; nh = (int)((double)S * ch / cw); }
    if (nh != ch || nw != cw) {
        std::vector<int> bh, kh, bv, kv;
        const int ksh = resample_coeffs(cw, nw, bh, kh), ksv = resample_coeffs(ch, nh, bv, kv);
        const size_t tab = bh.size() + kh.size() + bv.size() + kv.size();
        m->pp_tab.ensure(tab * 4);
        int* t = m->pp_tab.as<int>();
        int *d_bh = t, *d_kh = d_bh + bh.size(), *d_bv = d_kh + kh.size(), *d_kv = d_bv + bv.size();
        HIPCHK(hipMemcpyAsync(d_bh, bh.data(), bh.size() * 4, hipMemcpyHostToDevice, m->st));
        HIPCHK(hipMemcpyAsync(d_kh, kh.data(), kh.size() * 4, hipMemcpyHostToDevice, m->st));
        HIPCHK(hipMemcpyAsync(d_bv, bv.data(), bv.size() * 4, hipMemcpyHostToDevice, m->st));
        HIPCHK(hipMemcpyAsync(d_kv, kv.data(), kv.size() * 4, hipMemcpyHostToDevice, m->st));
        m->pp_tmp.ensure((size_t)ch * nw * 3);
        m->pp_out.ensure((size_t)nh * nw * 3);
        // PIL skips a pass whose size does not change, and runs horizontal first
        const uint8_t* src = cur;
        int th = ch;
        if (nw != cw) {
            launch_resample(src, ch, cw, m->pp_tmp.as<uint8_t>(), ch, nw, d_bh, d_kh, ksh, 1, m->st);
            src = m->pp_tmp.as<uint8_t>();
        }
        if (nh != ch) {
            launch_resample(src, th, nw, m->pp_out.as<uint8_t>(), nh, nw, d_bv, d_kv, ksv, 0, m->st);
            src = m->pp_out.as<uint8_t>();
        }
        cur = src;
        HIPCHK(hipStreamSynchronize(m->st));  // the host coefficient vectors go out of scope
    }
    const int top = (nh - S) / 2, left = (nw - S) / 2;
    float* dst = out;
    if (!out_on_device) {
        m->pp_f32.ensure((size_t)3 * S * S * 4);
        dst = m->pp_f32.as<float>();
    }
    launch_crop_normalize(cur, nh, nw, top, left, dst, S, mean, stdv, m->st);
    if (!out_on_device)
        HIPCHK(hipMemcpyAsync(out, dst, (size_t)3 * S * S * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    GUARD_END(m->ctx)
}

VC_API int vc_last_timings(vc_model* m, float* encode_ms, float* prefill_ms, float* decode_ms) {
    if (!m) return VC_ERR_INVALID;
    if (encode_ms) *encode_ms = m->t_encode;
    if (prefill_ms) *prefill_ms = m->t_prefill;
    if (decode_ms) *decode_ms = m->t_decode;
    return VC_OK;
}

/* times `reps` sweeps of the decode attention launches of one step (one per layer) over `B` rows at context `ctx` (keys per
 * row before the append; row b sits at ctx - (7 b) % 64 so the rows differ like concurrent requests do) with HIP events on the
 * model's stream; the KV contents are whatever the cache holds (the kernel's speed does not depend on the values).  Returns
 * launches per sweep, average microseconds per launch and the algorithmic KV bytes per launch (4 * sum(ctx_b + 1) * hidden). */
VC_API int vc_profile_decode_attention(vc_model* m, int B, int ctx, int reps, int* launches, double* avg_us, double* avg_bytes) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->finalized && B >= 1 && B <= VC_POOL_ROWS && reps >= 1 && ctx >= 64, VC_ERR_INVALID, "bad profile arguments");
    REQUIRE(m->precision == 0, VC_ERR_STATE, "the profile hooks time the bf16 path's kernels");
    const vc_model_cfg& c = m->c;
    LoopView v;
    if (B <= VC_MAX_ROWS) {
        ensure_llm(m, B, ctx + 64);
        v = session_view(m);
    } else {
        vc_pool* p = pool_for(m, ctx + 64, 1);
        pool_release(p);  // measurement hook: the caller guarantees that no generate() runs meanwhile
        {
            std::lock_guard<std::mutex> lk(p->mu);
            REQUIRE(p->users == 0 && p->active.empty() && p->pending.empty(), VC_ERR_STATE, "the decode pool is busy");
        }
        HIPCHK(hipStreamSynchronize(p->st));
        v = pool_view(p);
        v.st = m->st;
    }
    REQUIRE(ctx + 1 <= v.capS, VC_ERR_INVALID, "context %d exceeds the cache capacity %d", ctx, v.capS);
    v.split_G = 0;   // the sweep times the bf16 step's attention as such: no split group, no key mask
    v.kmask = nullptr;
    v.kmask_stride = 0;
    std::vector<int> rec((size_t)B * RS_STRIDE, 0);
    double keys = 0;
    for (int b = 0; b < B; ++b) {
        rec[(size_t)b * RS_STRIDE + RS_ACTIVE] = 1;
        rec[(size_t)b * RS_STRIDE + RS_POS] = ctx - (7 * b) % 64;
        keys += rec[(size_t)b * RS_STRIDE + RS_POS] + 1;
    }
    HIPCHK(hipMemcpyAsync(v.rows, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    auto sweep = [&]() {
        for (int l = 0; l < c.layers; ++l) {
            launch_attention_decode_fused(decode_attn_args(m, v, l, B), m->st);
        }
    };
    sweep();  // warm
    HIPCHK(hipEventRecord(m->ev[0], m->st));
    for (int r = 0; r < reps; ++r) sweep();
    HIPCHK(hipEventRecord(m->ev[1], m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
    if (launches) *launches = c.layers;
    if (avg_us) *avg_us = (double)ms * 1e3 / ((double)reps * c.layers);
    if (avg_bytes) *avg_bytes = 2.0 * (double)v.es * keys * (double)c.hidden;   // K + V rows of `es` bytes per element
    HIPCHK(hipMemsetAsync(v.rows, 0, (size_t)B * RS_STRIDE * 4, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    m->cur_pos = -1;
    GUARD_END(m->ctx)
}

/* cumulative number of pooled decode steps launched over 8, 16, 24 and 32 rows since the pool of m's root model was
 * created (zeros if it has none): lets bench.py weight the per-row-count kernel timings by what the timed run executed */
VC_API int vc_pool_step_counts(vc_model* m, unsigned long long* counts4) {
    if (!m || !counts4) return VC_ERR_INVALID;
    vc_model* root = root_of(m);
    for (int i = 0; i < 4; ++i) counts4[i] = 0;
    if (root->pool) {
        std::lock_guard<std::mutex> lk(root->pool->mu);
        for (int i = 0; i < 4; ++i) counts4[i] = root->pool->steps_by_span[i];
        // (a 64-row pool, vc_pool_set_rows: its steps over 40 .. 64 rows are reported with the 32-row count — two weight passes each)
        for (int i = 4; i < VC_POOL_ROWS_MAX / 8; ++i) counts4[3] += root->pool->steps_by_span[i];
    }
    return VC_OK;
}

/* In-situ timing of the pool's decode-step kernels.  on != 0: the pool's step graphs are (re)captured with a timing slot per launch
 * — the first thread of every workgroup stamps {earliest start, latest end} with the device's constant-rate wall clock — and one
 * tiny launch per step folds the slots into per-(span, kind) sums, so that a measurement covers every launch of a timed region as
 * it ran there (beside whatever the other sessions had on the GPU), not a replay.  Takes effect when the pool is next (re)built,
 * i.e. while it is idle.  bf16 path only (the split step keeps its graphs). */
/* Pool scheduling policy.  on = 1 (default): the pool does not launch a decode step while a generate() call that already holds
 * rows is still in its encode / prefill phase — it waits for that request to join (a step beside a prefill's GEMMs runs at a
 * fraction of its speed, and the joiner needs a full set of steps of its own anyway).  Throughput policy: the requests already
 * decoding see one pause of about a prefill when somebody joins.  on = 0: step whatever rows are active (lowest inter-token
 * latency for the requests in flight).  Applies to every session of the model. */
VC_API int vc_pool_set_hold(vc_model* m, int on) {
    if (!m) return VC_ERR_INVALID;
    vc_model* root = root_of(m);
    root->pool_hold.store(on != 0);
    // the pool may be rebuilt (destroyed and re-created) by pool_for under g_pool_create while this runs on another thread
    std::lock_guard<std::mutex> create_lk(g_pool_create);
    if (root->pool) {
        std::lock_guard<std::mutex> lk(root->pool->mu);
        root->pool->cv_driver.notify_all();
    }
    return VC_OK;
}

/* Rows of the decode pool: 32 (default; one weight pass per step: two MFMA token-slot groups) or 64 (measurement, round 6: a step
 * then takes TWO 32-row weight passes, i.e. what two 32-row pools would stream, plus the attention of 64 rows).  Takes effect when
 * the pool is next (re)built, i.e. while it is idle; a 64-row pool serves the bf16 step only and carries no in-situ timing slots. */
VC_API int vc_pool_set_rows(vc_model* m, int rows) {
    if (!m || (rows != VC_POOL_ROWS && rows != VC_POOL_ROWS_MAX)) return VC_ERR_INVALID;
    root_of(m)->pool_rows = rows;
    return VC_OK;
}

VC_API int vc_pool_profile(vc_model* m, int on) {
    if (!m) return VC_ERR_INVALID;
    vc_model* root = root_of(m);
    root->pool_profile = on != 0;
    return VC_OK;
}

/* sums since the last reset, for span s (8 (s + 1) rows) and kind k (0 qkv, 1 decode attention, 2 o_proj, 3 gate/up, 4 down,
 * 5 lm_head), each [4][6]: exec_us = earliest workgroup start -> latest workgroup end of the launches; period_us = latest end of
 * the previous launch of the step -> latest end of this one (dispatch, drain and the inter-kernel gap included: what the step's
 * dependency chain pays per launch); launches.  reset != 0 zeroes the sums.  The pool must be idle (no generate() in flight). */
VC_API int vc_pool_profile_read(vc_model* m, double* exec_us, double* period_us, unsigned long long* launches, int reset) {
    if (!m || !exec_us || !period_us || !launches) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    vc_model* root = root_of(m);
    const int nspan = VC_POOL_ROWS / 8;
    for (int i = 0; i < nspan * PROF_KINDS; ++i) {
        exec_us[i] = period_us[i] = 0;
        launches[i] = 0;
    }
    vc_pool* p = root->pool;
    if (p && p->prof) {
        {
            std::lock_guard<std::mutex> lk(p->mu);
            REQUIRE(p->users == 0 && p->active.empty() && p->pending.empty(), VC_ERR_STATE, "the decode pool is busy");
        }
        HIPCHK(hipStreamSynchronize(p->st));
        std::vector<unsigned long long> h((size_t)nspan * PROF_KINDS * 3);
        HIPCHK(hipMemcpy(h.data(), p->prof_acc.p, h.size() * 8, hipMemcpyDeviceToHost));
        int khz = 100000;   // the constant-rate wall clock: 100 MHz on gfx9
#ifndef VC_EMU
        (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, root->ctx->device);
        if (khz <= 0) khz = 100000;
#endif
        for (int i = 0; i < nspan * PROF_KINDS; ++i) {
            exec_us[i] = (double)h[3 * i] * 1e3 / (double)khz;
            period_us[i] = (double)h[3 * i + 1] * 1e3 / (double)khz;
            launches[i] = h[3 * i + 2];
        }
        if (reset) HIPCHK(hipMemset(p->prof_acc.p, 0, h.size() * 8));
    }
    GUARD_END(m->ctx)
}

VC_API int vc_profile_decode_gemv(vc_model* m, int B, int reps, int* launches, double* avg_us, double* avg_bytes) {
    if (!m) return VC_ERR_INVALID;
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(m->finalized && B >= 1 && B <= VC_POOL_ROWS && reps >= 1, VC_ERR_INVALID, "bad profile arguments");
    REQUIRE(m->precision == 0, VC_ERR_STATE, "the profile hooks time the bf16 path's kernels");
    const vc_model_cfg& c = m->c;
    const int D = c.hidden, F = c.ffn;
    LoopView v;
    if (B <= VC_MAX_ROWS) {
        ensure_llm(m, B, 64);
        v = session_view(m);
    } else {  // 17..32 rows: the decode pool's buffers (it must be idle), launches on this session's stream
        vc_pool* p = pool_for(m, 64, 1);
        pool_release(p);  // measurement hook: the caller guarantees that no generate() runs meanwhile
        {
            std::lock_guard<std::mutex> lk(p->mu);
            REQUIRE(p->users == 0 && p->active.empty() && p->pending.empty(), VC_ERR_STATE, "the decode pool is busy");
        }
        HIPCHK(hipStreamSynchronize(p->st));
        v = pool_view(p);
        v.st = m->st;
    }
    auto sweep = [&]() { decode_linears(m, v, B, [](int) {}); };
    sweep();  // warm
    HIPCHK(hipEventRecord(m->ev[0], m->st));
    for (int r = 0; r < reps; ++r) sweep();
    HIPCHK(hipEventRecord(m->ev[1], m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
    const int n = 4 * c.layers + 1;
    // bytes per decoder-linear weight (lm_head stays bf16); W4A16: a nibble + 1/32 of a scale byte
    const double wb = root_of(m)->weight_format == 3 ? 0.5 + 1.0 / 32.0 : m->weight_format >= 1 ? 1.0 : 2.0;
    const double bytes = wb * (double)c.layers * (4.0 * D * D + 3.0 * D * F) + 2.0 * (double)D * c.vocab;
    if (launches) *launches = n;
    if (avg_us) *avg_us = (double)ms * 1e3 / ((double)reps * n);
    if (avg_bytes) *avg_bytes = bytes / n;
    HIPCHK(hipMemsetAsync(v.x_dec, 0, (size_t)rup(B, 16) * D * 4, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    GUARD_END(m->ctx)
}

