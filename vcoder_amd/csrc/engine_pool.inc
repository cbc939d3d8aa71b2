// engine_pool.inc — part of the host engine (textually included by engine.hip): generate() — column trimming, the session's own hipGraph
// loop, the shared decode pool (driver thread, requests, hold policy), beam search inside the session's loop (vc_generate_beam) — and
// its C entry points.

namespace {

// first column count at which a row of `produced` ids is stopped by one of the stop sequences (host restatement of the
// select kernel's suffix match; used to trim the returned columns exactly where HF's loop would have stopped)
int row_stop_end(const GenParams& g, const int32_t* row, const int* tail_b, int produced) {
    constexpr int TL = VC_MAX_STOP_LEN - 1;
    for (int st = 0; st < produced; ++st)
        for (int i = 0; i < g.n_stop; ++i) {
            const int L = g.stop[i][0];
            bool ok = L > 0;
            for (int j = 0; j < L && ok; ++j) {
                const int back = L - 1 - j;
                const int v = st - back >= 0 ? row[st - back] : tail_b[TL + (st - back)];
                ok = v == g.stop[i][1 + j];
            }
            if (ok) return st + 1;
        }
    return produced;
}

// columns HF's loop would have returned: it stops right after the first step at which every row has produced EOS / met a stop
// columns of one row up to and including its finishing token (its EOS, or the token that completes a stop sequence); `produced`
// when the row never finished
int row_finish_end(const GenParams& g, const int32_t* row, const int* tail_b, int produced) {
    int e = produced;
    if (g.eos >= 0)
        for (int s_ = 0; s_ < produced; ++s_)
            if (row[s_] == g.eos) { e = s_ + 1; break; }
    if (g.n_stop > 0) e = std::min(e, row_stop_end(g, row, tail_b, produced));
    return e;
}
int trim_columns(const GenParams& g, const int32_t* out_ids, int ld, const int* tail, int B, int produced) {
    if (!(g.eos >= 0 || g.n_stop > 0)) return produced;
    int last = 0;
    for (int b = 0; b < B; ++b)
        last = std::max(last, row_finish_end(g, out_ids + (size_t)b * ld, tail + (size_t)b * (VC_MAX_STOP_LEN - 1), produced));
    return std::min(produced, last);
}

// one encode + prefill at a time PER PROCESS (two MFMA-bound phases side by side only slow each other down).  The deployment is
// one process per GPU (DESIGN.md section 7), so per process == per device; a process driving several devices would serialise their
// prefills' ENQUEUEING here (not their execution) and should then gate per device instead.
std::mutex g_prefill_gate;

// =================================================================================================
// Decode pool: the cached decode steps of CONCURRENT generate() calls share one step.
//
// A decode step streams every decoder weight once whatever the number of rows in it (<= 32: two MFMA token-slot groups
// per weight tile), so k requests decoding side by side on private loops read the weights k times per token where one
// pooled step reads them once — the HBM leg of the composite roofline per image drops from  W + KV  to  W / k + KV
// (DESIGN.md section 2b).  The reference's callers issue independent generate() calls (serve/cli.py:122, the eval
// loaders' per-sample loop, one process per GPU in scripts/v1_5/eval/cost_depth.sh); the pool is what lets several of them
// in flight on one GPU behave like one larger batch during decode without changing what any of them computes: rows are
// independent in every kernel of the step, a row's arithmetic does not depend on which other rows are present, and the
// ids a request gets are bit-identical to the ones its own loop would produce (tests: pooled == session loop).
//
//   request thread (vc_generate)                         driver thread (one per pool)
//   ---------------------------------------------       ---------------------------------------------------------------
//   take B free rows of the pool                         loop:
//   encode + prefill on ITS stream, keys / values          admit pending requests between two steps: wait for their prefill
//     written straight into the pool's KV rows               event on the pool stream, write their RowState records, select
//   record prefill-done event, queue the request             token 0 from the request's prefill logits (select kernel)
//   sleep until done (streaming: wake per report)          replay the step graph over the first 16 / all 32 rows
//   copy its out_ids rows, free the rows                    count steps per request; retire finished ones (rows inactive)
//
// Only the driver touches the pool's decode state, always on the pool's stream, so joins and retirements are ordered
// between steps without any host synchronisation of the GPU; the only host waits are a bounded run-ahead (two steps) and
// the completion events the request threads sleep on.
struct PoolRequest {
    vc_model* sess = nullptr;
    int row0 = 0, B = 0;
    GenParams g;
    std::vector<int> tail;
    int* rec = nullptr;               // pinned host copy of the B RowState records
    hipEvent_t prefill_done = nullptr, join_ev = nullptr, done_ev = nullptr, report_ev = nullptr;
    int steps_left = 0;               // pool steps still to run for it
    int produced = 0;                 // columns of out_ids written so far (driver's count)
    bool can_finish = false;
    // early finish poll (EOS / stops): FINISHED words copied out asynchronously
    int* fin_host = nullptr;          // pinned [B]
    hipEvent_t fin_ev = nullptr;
    bool fin_pending = false;
    int fin_at = 0;                   // `produced` at the time the poll was issued
    // hand-off to the request thread
    bool done = false, failed = false;
    std::string err;
    int avail = 0;                    // columns the request thread may read (streaming)
    bool report_taken = true;
    vc_token_cb cb = nullptr;
    int cb_every = 1;
    std::condition_variable cv;
};

}  // namespace

struct vc_pool {
    vc_model* root = nullptr;
    int device = 0;
    hipStream_t st = nullptr;
    int R = VC_POOL_ROWS, capS = 0, out_stride = 0;   // R: rows of THIS pool (root->pool_rows when it was built)
    bool split = false;               // built for precision mode "split": fp32 KV, stacked hi / lo step operands
    int kv_es = 2;                    // bytes per cache element: 2 bf16, 1 e4m3 (fp8 weight format), 3 / 4 fp24 / fp32 (split)
    int split_G = 16;                 // rows per stacked hi / lo group: 16 (per-wave-ring GEMV: two weight passes per 32-row step)
                                      // or 32 (workgroup-shared GEMV: one)
    Buf kc, vc, rows, x_dec, xg_dec, qkv_dec, attn_dec, h_dec, logits, next_tok, out_ids, ssq, sk_scratch, sk_counters;
    hipGraphExec_t graph[VC_POOL_ROWS_MAX / 8] = {};    // one decode step over rows [0, 8 * (i + 1))
    std::mutex mu;
    std::condition_variable cv_driver, cv_rows;
    std::deque<PoolRequest*> pending;
    std::vector<PoolRequest*> active;
    bool used[VC_POOL_ROWS_MAX] = {};
    int users = 0;                    // generate() calls inside the pool (rows held or waited for)
    bool stop = false;
    std::thread driver;
    hipEvent_t step_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned long steps_run = 0;
    unsigned long long steps_by_span[VC_POOL_ROWS_MAX / 8] = {};  // steps launched over 8 / 16 / 24 / 32 (... 64) rows (vc_pool_step_counts)
    // generate() calls that hold rows and have not yet handed their request to the driver (encode + prefill being enqueued): with
    // the hold policy (vc_pool_set_hold) the driver waits for them instead of stepping the rows it has — a step that runs beside a
    // prefill's GEMMs takes 2-7x its time (profiles/r05_d_decode_kernels_alone_vs_corun.md) and the joiner needs a full set of
    // steps of its own anyway, so nothing is gained by starting without it
    int prefilling = 0;
    // in-situ timing (vc_pool_profile): the step graphs were captured with stamp slots; prof_acc[span][kind] = {exec ticks,
    // period ticks, launches}
    bool prof = false;
    Buf stamps, prof_acc, stamp_scratch;
};

namespace {

LoopView pool_view(vc_pool* p) {
    LoopView v{};
    v.st = p->st;
    v.kc = p->kc.as<bf16_t>();
    v.vc = p->vc.as<bf16_t>();
    v.es = p->kv_es;
    // one layout whatever rows a step spans: a row keeps its slot between steps.  The workgroup-shared GEMV takes all 32 rows
    // (hi + lo planes) in ONE weight pass; the per-wave-ring form two passes of 16
    v.split_G = p->split ? p->split_G : 0;
    v.capR = p->R;
    v.capS = p->capS;
    v.rows = p->rows.as<int>();
    v.x_dec = p->x_dec.as<float>();
    v.xg_dec = p->xg_dec.as<bf16_t>();
    v.qkv_dec = p->qkv_dec.as<bf16_t>();
    v.attn_dec = p->attn_dec.as<bf16_t>();
    v.h_dec = p->h_dec.as<bf16_t>();
    v.logits = p->logits.as<float>();
    v.next_tok = p->next_tok.as<int>();
    v.out_ids = p->out_ids.as<int>();
    v.ssq = p->ssq.as<float>();
    v.sk_scratch = p->sk_scratch.as<float>();
    v.sk_counters = p->sk_counters.as<unsigned>();
    v.stamps = p->prof ? p->stamps.as<unsigned>() : nullptr;
    v.stamp_scratch = p->prof ? p->stamp_scratch.as<unsigned>() : nullptr;
    return v;
}

void pool_retire(vc_pool* p, PoolRequest* rq, bool failed, const std::string& err) {  // p->mu held
    rq->done = true;
    rq->failed = failed;
    rq->err = err;
    rq->avail = rq->produced;
    rq->cv.notify_all();
}

void pool_fail_all(vc_pool* p, const std::string& msg) {  // p->mu held
    for (PoolRequest* rq : p->active) pool_retire(p, rq, true, msg);
    for (PoolRequest* rq : p->pending) pool_retire(p, rq, true, msg);
    p->active.clear();
    p->pending.clear();
    p->stop = true;
}

void pool_driver(vc_pool* p) {
    (void)hipSetDevice(p->device);
    t_stream = p->st;
    const LoopView v = pool_view(p);
    vc_model* m = p->root;
    std::unique_lock<std::mutex> lk(p->mu);
    try {
        for (;;) {
            p->cv_driver.wait(lk, [&] { return p->stop || !p->pending.empty() || !p->active.empty(); });
            if (p->stop) break;
            // ---- admit: everything is enqueued on the pool stream between two steps
            while (!p->pending.empty()) {
                PoolRequest* rq = p->pending.front();
                p->pending.pop_front();
                HIPCHK(hipStreamWaitEvent(p->st, rq->prefill_done, 0));
                HIPCHK(hipMemcpyAsync(v.rows + (size_t)rq->row0 * RS_STRIDE, rq->rec, (size_t)rq->B * RS_STRIDE * 4,
                                      hipMemcpyHostToDevice, p->st));
                HIPCHK(hipEventRecord(rq->join_ev, p->st));
                SelectArgs sa = select_args(m, v, rq->sess->logits.as<float>(), rq->B, 1);  // token 0: step 0 -> 1, position stays
                sa.row0 = rq->row0;
                launch_select_embed(sa, p->st);
                rq->produced = 1;
                rq->steps_left = rq->g.max_new - 1;
                p->active.push_back(rq);
            }
            // ---- retire requests that need no (further) step, before and after stepping
            auto retire_finished = [&]() {
                for (size_t i = 0; i < p->active.size();) {
                    PoolRequest* rq = p->active[i];
                    bool over = rq->steps_left <= 0;
                    if (!over && rq->fin_pending && hipEventQuery(rq->fin_ev) == hipSuccess) {
                        rq->fin_pending = false;
                        bool all = true;
                        for (int b = 0; b < rq->B; ++b) all = all && rq->fin_host[b] != 0;
                        if (all) {  // every row had finished when the poll was taken: later columns are pads
                            rq->produced = std::min(rq->produced, std::max(rq->fin_at, 1));
                            over = true;
                        }
                    }
                    if (!over) { ++i; continue; }
                    // rows go inactive (RS_ACTIVE is word 0 of each record), stream-ordered after the request's last step
                    HIPCHK(hipMemset2DAsync(v.rows + (size_t)rq->row0 * RS_STRIDE, (size_t)RS_STRIDE * 4, 0, 4, rq->B, p->st));
                    HIPCHK(hipEventRecord(rq->done_ev, p->st));
                    p->active.erase(p->active.begin() + i);
                    pool_retire(p, rq, false, "");
                }
            };
            retire_finished();
            if (p->active.empty()) continue;
            if (p->root->pool_hold.load() && p->prefilling > 0) {
                // somebody is about to join: wait for its request (or for it to give up) rather than step without it
                // (a request cancelled by its caller — steps_left forced to 0, generate_on_pool's failure path — ends the wait too:
                // the loop's next pass retires it instead of keeping its caller blocked for somebody else's whole prefill)
                p->cv_driver.wait(lk, [&] {
                    bool cancelled = false;
                    for (PoolRequest* rq : p->active) cancelled = cancelled || rq->steps_left <= 0;
                    return p->stop || !p->pending.empty() || p->prefilling == 0 || !p->root->pool_hold.load() || cancelled;
                });
                continue;
            }
            int top = 0;
            for (PoolRequest* rq : p->active) top = std::max(top, rq->row0 + rq->B);
            const int gi = (top + 7) / 8 - 1;  // the step covers rows [0, top) rounded up to 8: free rows above cost nothing
            // bounded run-ahead: at most two steps queued beyond the one executing (a joining request waits that long)
            const unsigned long n = p->steps_run;
            if (n >= 2) {
                hipEvent_t e = p->step_ev[(n - 2) % 4];
                lk.unlock();
                HIPCHK(hipEventSynchronize(e));
                lk.lock();
            }
            HIPCHK(hipGraphLaunch(p->graph[gi], p->st));
            HIPCHK(hipEventRecord(p->step_ev[n % 4], p->st));
            p->steps_run = n + 1;
            p->steps_by_span[gi] += 1;
            for (PoolRequest* rq : p->active) {
                rq->steps_left -= 1;
                rq->produced += 1;
                // streamer: hand the request thread an event every cb_every columns (skipped while it is still busy)
                if (rq->cb && rq->report_taken && rq->produced - rq->avail >= rq->cb_every && rq->steps_left > 0) {
                    HIPCHK(hipEventRecord(rq->report_ev, p->st));
                    rq->avail = rq->produced;
                    rq->report_taken = false;
                    rq->cv.notify_all();
                }
                // EOS / stop: look at the rows' FINISHED words every 8 columns without stalling the stream
                if (rq->can_finish && !rq->fin_pending && rq->produced % 8 == 0 && rq->steps_left > 0) {
                    HIPCHK(hipMemcpy2DAsync(rq->fin_host, 4, v.rows + (size_t)rq->row0 * RS_STRIDE + RS_FINISHED,
                                            (size_t)RS_STRIDE * 4, 4, rq->B, hipMemcpyDeviceToHost, p->st));
                    HIPCHK(hipEventRecord(rq->fin_ev, p->st));
                    rq->fin_pending = true;
                    rq->fin_at = rq->produced;
                }
            }
            retire_finished();
        }
    } catch (const Fail& f) {
        pool_fail_all(p, f.msg);
    } catch (const std::exception& e) {  // a refused kernel launch
        pool_fail_all(p, e.what());
    }
}

void pool_destroy(vc_pool* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->stop = true;
    }
    p->cv_driver.notify_all();
    if (p->driver.joinable()) p->driver.join();
    (void)hipSetDevice(p->device);
    if (p->st) (void)hipStreamSynchronize(p->st);
    for (auto& g : p->graph)
        if (g) (void)hipGraphExecDestroy(g);
    for (Buf* b : {&p->kc, &p->vc, &p->rows, &p->x_dec, &p->xg_dec, &p->qkv_dec, &p->attn_dec, &p->h_dec, &p->logits,
                   &p->next_tok, &p->out_ids, &p->ssq, &p->sk_scratch, &p->sk_counters, &p->stamps, &p->prof_acc, &p->stamp_scratch})
        b->release();
    for (auto& e : p->step_ev)
        if (e) (void)hipEventDestroy(e);
    if (p->st) (void)hipStreamDestroy(p->st);
    delete p;
}

std::mutex g_pool_create;

// rows per stacked hi / lo group of a split pool: 32 when the workgroup-shared GEMV (one weight pass over the 32 rows' two planes)
// can serve EVERY matrix of the model, else the per-wave-ring form's two passes of 16
int pool_split_G(const vc_model* root) {
    const vc_model_cfg& c = root->c;
    const bool fp8w = root->weight_format != 0;   // (W4A16 included: like the e4m3 formats it is served by per-wave rings only)
    return (gemv_wg_enabled() && gemv_wg_applies(c.hidden, fp8w) && gemv_wg_applies(c.ffn, fp8w)) ? 32 : 16;
}

// the root model's pool with room for `need_S` positions and `need_out` ids per row; an idle pool that is too small (or that
// stopped after an error) is rebuilt, a busy one makes the caller wait for it to drain.  The pool is returned ACQUIRED:
// p->users was incremented while g_pool_create was still held, so no concurrent pool_for can find it idle and destroy it
// before the caller has registered (callers release with pool_release).
// whether a pool built now for `root` carries the in-situ timing slots: asked for, a bf16-step pool (a split step's GEMVs may take
// two passes: the slot layout assumes one — as do the two weight passes of a 64-row pool), and within the fold kernel's 512 slots.
// ONE definition for the rebuild test and the build (ADVICE r5: with the slot limit missing from the test, a > 102-layer model
// with profiling on would have rebuilt its pool on every generate()).
bool pool_wants_prof(const vc_model* root, bool want_split) {
    return root->pool_profile && !want_split && root->pool_rows <= VC_POOL_ROWS && 5 * root->c.layers + 1 <= 512;
}

vc_pool* pool_for(vc_model* m, int need_S, int need_out) {
    vc_model* root = root_of(m);
    const vc_model_cfg& c = root->c;
    std::unique_lock<std::mutex> create(g_pool_create);
    vc_pool* p = root->pool;
    const bool want_split = m->precision == 2;
    if (p) {
        std::unique_lock<std::mutex> lk(p->mu);
        // (a split pool laid out for the other GEMV form — set_gemv_variant switched since it was built — is rebuilt as well)
        if (p->capS < need_S || p->out_stride < need_out || p->stop || p->split != want_split ||
            (want_split && p->split_G != pool_split_G(root)) || p->prof != pool_wants_prof(root, want_split) || p->R != root->pool_rows) {
            p->cv_rows.wait(lk, [&] { return p->users == 0; });
            lk.unlock();
            pool_destroy(p);
            root->pool = p = nullptr;
        } else {
            p->users += 1;
            return p;
        }
    }
    p = new vc_pool();
    try {
        p->root = root;
        p->device = root->ctx->device;
        p->split = want_split;
        p->split_G = pool_split_G(root);
        p->R = root->pool_rows;
        REQUIRE(!(want_split && p->R > VC_POOL_ROWS), VC_ERR_STATE, "a %d-row pool serves the bf16 step only", p->R);
        const int D = c.hidden, F = c.ffn, H = c.heads, R = p->R;
        const size_t es = want_split ? (size_t)split_kv_es() : (size_t)step_kv_es(root), two = want_split ? 2 : 1;
        p->kv_es = (int)es;
        p->capS = std::min((int)rup(std::max(need_S, 2048), 64), c.max_positions / 64 * 64);
        p->out_stride = std::max(need_out, p->capS);
        REQUIRE(p->capS >= need_S, VC_ERR_INVALID, "sequence %d exceeds max_position_embeddings=%d", need_S, c.max_positions);
        p->st = make_stream();
        t_stream = p->st;  // zero-fills of the new buffers
        const size_t kvb = (size_t)c.layers * R * H * p->capS * root->hd * es;
        p->kc.ensure(kvb, true);
        p->vc.ensure(kvb, true);
        p->rows.ensure((size_t)R * RS_STRIDE * 4, true);
        p->x_dec.ensure((size_t)R * D * 4, true);
        p->xg_dec.ensure(two * R * D * 2, true);
        p->qkv_dec.ensure((size_t)R * 3 * D * (want_split ? 4 : 2), true);   // the split step's projection rows are fp32
        p->attn_dec.ensure(two * R * D * 2, true);
        p->h_dec.ensure(two * R * F * 2, true);
        p->logits.ensure((size_t)R * c.vocab * 4, true);
        p->next_tok.ensure(R * 4, true);
        p->out_ids.ensure((size_t)R * p->out_stride * 4, true);
        p->ssq.ensure((size_t)R * root->npart * 4, true);
        p->sk_scratch.ensure(sk_floats(c) * 4);   // [K-slices][tiles][2 row groups][256]
        p->sk_counters.ensure((size_t)sk_counters_n(c) * 4, true);
        t_stream = m->st;
        for (auto& e : p->step_ev) HIPCHK(hipEventCreate(&e));
        // (a split step's GEMVs may take two passes: the slot layout assumes one; the fold kernel walks at most 512 slots)
        p->prof = pool_wants_prof(root, want_split);
        if (p->prof) {
            const size_t nslots = (size_t)5 * c.layers + 1;
            p->stamps.ensure(nslots * STAMP_SLOT_WORDS * 4, true);
            p->prof_acc.ensure((size_t)(R / 8) * PROF_KINDS * 3 * 8, true);
            p->stamp_scratch.ensure((1 + 2 * nslots) * 4, true);
            HIPCHK(hipStreamSynchronize(m->st));
        }
        LoopView v = pool_view(p);
        for (int i = 0; i < R / 8; ++i) {
            int slot = 0;
            if (p->prof) {
                v.stamp_next = &slot;
                v.prof_acc = p->prof_acc.as<unsigned long long>() + (size_t)i * PROF_KINDS * 3;
            }
            p->graph[i] = capture_step(root, v, 8 * (i + 1));
        }
        p->driver = std::thread(pool_driver, p);
    } catch (...) {  // a failed allocation / capture must not leak the half-built pool or leave t_stream on its stream
        t_stream = m->st;
        pool_destroy(p);
        throw;
    }
    p->users = 1;
    root->pool = p;
    return p;
}
void pool_release(vc_pool* p) {
    std::lock_guard<std::mutex> lk(p->mu);
    p->users -= 1;
    p->cv_rows.notify_all();
}

// generate() through the pool: prefill on the session's stream into pool rows, decode steps shared with whoever else is in
#define DBG_HIP(tag)                                                                                         \
    do {                                                                                                     \
        if (g_dbg_hip) {                                                                                     \
            hipError_t e_ = hipGetLastError();                                                               \
            if (e_ != hipSuccess) fprintf(stderr, "[vcoder_amd] last-error %d (%s) after %s\n", (int)e_, hipGetErrorString(e_), tag); \
        }                                                                                                    \
    } while (0)
const bool g_dbg_hip = getenv("VC_DEBUG_HIP") != nullptr;

// the epilogue of every generate call: the phase times of the call that just ended, its decode phase between the two events given
void read_phase_times(vc_model* m, hipEvent_t decode_begin, hipEvent_t decode_end) {
    if (!m->ev[0]) return;
    (void)hipEventElapsedTime(&m->t_encode, m->ev[0], m->ev[1]);
    (void)hipEventElapsedTime(&m->t_prefill, m->ev[1], m->ev[2]);
    (void)hipEventElapsedTime(&m->t_decode, decode_begin, decode_end);
}

void generate_on_pool(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                      int on_dev, const GenParams& g, const std::vector<int>& tail, vc_token_cb cb, void* cb_user,
                      int cb_every, int32_t* out_ids, int* n_generated) {
    const vc_model_cfg& c = m->c;
    const int max_new = g.max_new;
    // the spliced length is only known after the splice plan; an upper bound sizes the pool: the text rows plus one
    // feature block per image the sample owns (vc_set_image_counts: the list / 5-D form gives a sample several images per
    // modality; otherwise one per modality), over the sample with the most images
    int n_img_max = 3;
    for (int b = 0; b < B; ++b) {
        int n_b = 0;
        for (int k = 0; k < 3; ++k) n_b += m->img_counts[k].empty() ? 1 : ((int)m->img_counts[k].size() == B ? m->img_counts[k][b] : 1);
        n_img_max = std::max(n_img_max, n_b);
    }
    const int S_bound = std::min(c.max_positions, T + n_img_max * m->Tv);
    vc_pool* p = pool_for(m, std::min(S_bound + max_new, c.max_positions / 64 * 64), max_new);  // acquired: users counted
    PoolRequest rq;
    rq.sess = m;
    rq.B = B;
    rq.g = g;
    rq.tail = tail;
    rq.cb = cb;
    rq.cb_every = std::max(cb_every, 1);
    rq.can_finish = g.eos >= 0 || g.n_stop > 0;
    // ---- rows: first fit of B contiguous free rows; blocks while the pool is full
    {
        std::unique_lock<std::mutex> lk(p->mu);
        int row0 = -1;
        p->cv_rows.wait(lk, [&] {
            for (int r0 = 0; r0 + B <= p->R; ++r0) {
                bool free_ = true;
                for (int r = r0; r < r0 + B && free_; ++r) free_ = !p->used[r];
                if (free_) { row0 = r0; return true; }
            }
            return false;
        });
        for (int r = row0; r < row0 + B; ++r) p->used[r] = true;
        rq.row0 = row0;
        p->prefilling += 1;
    }
    bool counted_prefilling = true;
    auto done_prefilling = [&]() {   // p->mu held
        if (!counted_prefilling) return;
        counted_prefilling = false;
        p->prefilling -= 1;
        p->cv_driver.notify_all();
    };
    auto release_rows = [&]() {
        std::lock_guard<std::mutex> lk(p->mu);
        for (int r = rq.row0; r < rq.row0 + B; ++r) p->used[r] = false;
        p->users -= 1;
        p->cv_rows.notify_all();
    };
    hipEvent_t* evs[] = {&rq.prefill_done, &rq.join_ev, &rq.done_ev, &rq.report_ev, &rq.fin_ev};
    auto cleanup = [&]() {
        for (hipEvent_t* e : evs)
            if (*e) (void)hipEventDestroy(*e);
        if (rq.rec) (void)hipHostFree(rq.rec);
        if (rq.fin_host) (void)hipHostFree(rq.fin_host);
    };
    try {
        for (hipEvent_t* e : evs) HIPCHK(hipEventCreate(e));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&rq.rec), (size_t)B * RS_STRIDE * 4, 0));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&rq.fin_host), (size_t)B * 4, 0));
        DBG_HIP("pool request setup");
        // ---- encode + prefill, keys / values straight into the pool's rows
        m->cur_pos = -1;
        int S = 0;
        std::unique_lock<std::mutex> gate(g_prefill_gate);
        do_prefill(m, ids, B, T, img, seg, depth, on_dev, 1, max_new, false, &S);
        DBG_HIP("do_prefill");
        m->last_S = S;
        REQUIRE(S + max_new <= p->capS, VC_ERR_INVALID,
                "prompt %d + max_new %d exceeds the context: max_position_embeddings=%d (KV capacity %d)", S, max_new,
                m->c.max_positions, p->capS);
        finish_prefill(m, KvTarget{p->kc.as<bf16_t>(), p->vc.as<bf16_t>(), p->R, p->capS, rq.row0, p->kv_es}, nullptr);
        if (m->ev[2]) HIPCHK(hipEventRecord(m->ev[2], m->st));
        HIPCHK(hipEventRecord(rq.prefill_done, m->st));
        DBG_HIP("finish_prefill");
        gate.unlock();
        fill_rows(rq.rec, B, g, S, tail.data(), rq.row0 * p->out_stride, p->out_stride);
        // ---- join, then sleep until the driver retires the request (streaming: wake per report)
        std::unique_lock<std::mutex> lk(p->mu);
        REQUIRE(!p->stop, VC_ERR_STATE, "the decode pool has stopped after an error");
        p->pending.push_back(&rq);
        done_prefilling();
        p->cv_driver.notify_all();
        int reported = 0;
        std::vector<int> part;
        auto report = [&](int upto, hipEvent_t after) {  // called with lk held; drops it around the copy + callback
            if (!cb || upto <= reported) return;
            lk.unlock();
            HIPCHK(hipStreamWaitEvent(m->st, after, 0));
            part.resize((size_t)B * (upto - reported));
            HIPCHK(hipMemcpy2DAsync(part.data(), (size_t)(upto - reported) * 4,
                                    p->out_ids.as<int>() + (size_t)rq.row0 * p->out_stride + reported,
                                    (size_t)p->out_stride * 4, (size_t)(upto - reported) * 4, B, hipMemcpyDeviceToHost, m->st));
            HIPCHK(hipStreamSynchronize(m->st));
            cb(cb_user, reported, upto - reported, B, part.data());
            reported = upto;
            lk.lock();
        };
        for (;;) {
            rq.cv.wait(lk, [&] { return rq.done || !rq.report_taken; });
            if (rq.done) break;
            const int upto = rq.avail;
            report(upto, rq.report_ev);
            rq.report_taken = true;
        }
        REQUIRE(!rq.failed, VC_ERR_HIP, "decode pool: %s", rq.err.c_str());
        int produced = rq.produced;
        lk.unlock();
        HIPCHK(hipStreamWaitEvent(m->st, rq.done_ev, 0));
        HIPCHK(hipMemcpy2DAsync(out_ids, (size_t)max_new * 4, p->out_ids.as<int>() + (size_t)rq.row0 * p->out_stride,
                                (size_t)p->out_stride * 4, (size_t)max_new * 4, B, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        DBG_HIP("pool result copy");
        for (int b = 0; b < B; ++b)  // columns the loop never reached read as pad, like the session loop's pre-filled store
            for (int s_ = produced; s_ < max_new; ++s_) out_ids[(size_t)b * max_new + s_] = g.pad;
        produced = trim_columns(g, out_ids, max_new, tail.data(), B, produced);
        if (cb && produced > reported) {
            part.resize((size_t)B * (produced - reported));
            for (int b = 0; b < B; ++b)
                memcpy(part.data() + (size_t)b * (produced - reported), out_ids + (size_t)b * max_new + reported,
                       (size_t)(produced - reported) * 4);
            cb(cb_user, reported, produced - reported, B, part.data());
        }
        if (n_generated) *n_generated = produced;
        read_phase_times(m, rq.join_ev, rq.done_ev);
        DBG_HIP("pool timings");
    } catch (...) {
        {   // a request that is still queued / active must not outlive this frame
            std::unique_lock<std::mutex> lk(p->mu);
            done_prefilling();
            auto it = std::find(p->pending.begin(), p->pending.end(), &rq);
            if (it != p->pending.end()) p->pending.erase(it);
            else if (!rq.done && std::find(p->active.begin(), p->active.end(), &rq) != p->active.end()) {
                rq.steps_left = 0;  // the driver retires it at its next pass
                p->cv_driver.notify_all();
                rq.cv.wait(lk, [&] { return rq.done; });
            }
        }
        (void)hipStreamSynchronize(m->st);
        release_rows();
        cleanup();
        throw;
    }
    release_rows();
    cleanup();
}


// The prologue of a generate call on the session's own loop: encode + splice + prefill with room for max_new steps, the loop's
// decode steps under an all-ones mask, the end of the prefill phase recorded (ev[2]).  -> the prefill gate, still held: the caller
// releases it behind its step-0 selection.  m->last_S = the spliced length.
std::unique_lock<std::mutex> prefill_on_session(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                                                const float* depth, int on_dev, int max_new) {
    m->cur_pos = -1;
    int S = 0;
    // Sessions of one process take turns in the MFMA-bound encode+prefill phase: two prefills side by side only slow
    // each other (and every decode in flight), while ONE prefill overlaps well with the HBM-bound decodes of the others.
    std::unique_lock<std::mutex> gate(g_prefill_gate);
    do_prefill(m, ids, B, T, img, seg, depth, on_dev, 1, max_new, true, &S);  // generate() always builds a mask
    m->last_S = S;
    REQUIRE(S + max_new <= m->capS, VC_ERR_INVALID, "prompt %d + max_new %d exceeds the KV capacity %d", S, max_new, m->capS);
    finish_prefill(m, session_kv(m), nullptr);
    m->kmask_in_decode = false;   // generate(): the cached steps run under an all-ones mask (vcoder_ds_llava_arch.py:130-133)
    if (m->ev[2]) HIPCHK(hipEventRecord(m->ev[2], m->st));
    return gate;
}

// the guidance request a call serves (vc_request_guidance), taken out of the model before anything can fail
struct GuidanceCall {
    float scale = 1.f;
    std::vector<int64_t> ids;   // the negative prompt [B, T]
    int B = 0, T = 0, on_dev = 0;
    const float* px[3] = {nullptr, nullptr, nullptr};
};
GuidanceCall take_guidance(vc_model* m) {
    GuidanceCall gd;
    gd.scale = m->gd_scale;
    gd.ids.swap(m->gd_ids);
    gd.B = m->gd_B;
    gd.T = m->gd_T;
    gd.on_dev = m->gd_px_on_dev;
    for (int k = 0; k < 3; ++k) gd.px[k] = m->gd_px[k];
    clear_guidance_request(m);
    return gd;
}

// The two prompts of a guided call on the session's own loop of R = 2 B rows: the negative prompt is prefilled straight into cache
// rows B .. 2 B - 1 (KvTarget::row0, as a request joins the pool's cache) and its last-row logits moved up by B rows, then the caller's
// prompt into rows 0 .. B - 1 — two prefills of B rows each, so each has the bits a call of its own gives it (one prefill of 2 B rows
// would not: README, batch invariance).  Both spliced lengths are planned first (do_prefill's plan_only form: no tower pass, no state),
// so the first prefill already sizes the cache for max(S_c, S_n) + `room` positions and the second cannot re-allocate it.  The
// caller's attention mask and image counts belong to ITS prompt; the negative prompt is rectangular with one image per placeholder.
// hint: `room` is a wish (vc_prefill's reserve), cut at max_position_embeddings; else required (generate's max_new).
std::unique_lock<std::mutex> prefill_guided_on_session(vc_model* m, const GuidanceCall& gd, const int64_t* ids, int B, int T,
                                                       const float* img, const float* seg, const float* depth, int on_dev, int has_mask,
                                                       int room, bool hint, int* S_c_out, int* S_n_out) {
    const int R = 2 * B;
    std::vector<int> counts[3];
    for (int k = 0; k < 3; ++k) counts[k] = m->img_counts[k];
    int S_c = 0, S_n = 0;
    {
        struct Plan {
            vc_model* m;
            ~Plan() { m->plan_only = false; }
        } plan{m};
        m->plan_only = true;
        do_prefill(m, ids, B, T, img, seg, depth, on_dev, has_mask, -1, false, &S_c);   // (consumes the image counts, not the mask)
        do_prefill(m, gd.ids.data(), B, gd.T, gd.px[0], gd.px[1], gd.px[2], gd.on_dev, has_mask, -1, false, &S_n);
    }
    m->cur_pos = -1;   // from here on the cache is being overwritten: a call that fails half-way leaves no loop to step
    int total = std::max(S_c, S_n) + std::max(room, 1);
    if (hint) total = std::max(std::max(S_c, S_n) + 1, std::min(total, m->c.max_positions / 64 * 64));
    std::vector<uint8_t> mask;
    mask.swap(m->mask_next);
    std::unique_lock<std::mutex> gate(g_prefill_gate);
    struct Rows {
        vc_model* m;
        ~Rows() { m->fan_rows = 0; }
    } rows{m};
    m->fan_rows = R;   // both prefills size the cache and the loop's buffers for R rows
    int S = 0;
    do_prefill(m, gd.ids.data(), B, gd.T, gd.px[0], gd.px[1], gd.px[2], gd.on_dev, has_mask, total - S_n, true, &S);
    REQUIRE(S == S_n && m->capB == R && total <= m->capS, VC_ERR_STATE, "guided prefill: planned %d rows, spliced %d (cache %d x %d)", S_n, S,
            m->capB, m->capS);
    finish_prefill(m, KvTarget{m->kc.as<bf16_t>(), m->vc.as<bf16_t>(), m->capB, m->capS, B, m->kv_es}, nullptr);
    const size_t lg = (size_t)B * m->c.vocab * 4;
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char*>(m->logits.p) + lg, m->logits.p, lg, hipMemcpyDeviceToDevice, m->st));
    const void* kc0 = m->kc.p;
    const int capS0 = m->capS;
    for (int k = 0; k < 3; ++k) m->img_counts[k] = counts[k];
    m->mask_next.swap(mask);
    do_prefill(m, ids, B, T, img, seg, depth, on_dev, has_mask, total - S_c, true, &S);
    REQUIRE(S == S_c && m->kc.p == kc0 && m->capS == capS0 && m->capB == R, VC_ERR_STATE,
            "guided prefill: the second prompt moved the cache (planned %d rows, spliced %d)", S_c, S);
    finish_prefill(m, session_kv(m), nullptr);
    m->last_S = S_c;
    m->kmask_in_decode = false;   // the cached steps of both streams run under an all-ones mask, as generate()'s
    if (m->ev[2]) HIPCHK(hipEventRecord(m->ev[2], m->st));
    if (S_c_out) *S_c_out = S_c;
    if (S_n_out) *S_n_out = S_n;
    return gate;
}

// vc_prefill with a pending vc_request_guidance (every precision mode: the strict prefill takes the row offset, the strict step the
// rows' own positions — run_llm_layers_strict): the same state of 2 B rows for a host loop — logits_last [2 B, V] (the conditional
// rows, then the negative prompts'), and a loop vc_decode_step steps over 2 B host-supplied tokens (the pairs advance their own
// positions; nothing is selected on the device: vc_decode_step(tok = NULL) is refused as behind a rewind)
void guided_prefill(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth, int on_dev,
                    int has_mask, float* logits_last, int* S_out) {
    const GuidanceCall gd = take_guidance(m);
    int S_c = 0, S_n = 0;
    std::unique_lock<std::mutex> gate = prefill_guided_on_session(m, gd, ids, B, T, img, seg, depth, on_dev, has_mask, m->reserve_new, true, &S_c, &S_n);
    ensure_out_ids(m, 2 * B, 1);
    GenParams g;   // nothing is recorded (max_new 0), no EOS bookkeeping
    arm_guided_rows(m, g, nullptr, B, S_c, S_n, gd.scale);
    m->curB = 2 * B;
    m->gd_pair = B;
    m->tok_stale = true;
    m->gd_last = true;
    m->gd_last_B = B;
    m->gd_last_Sc = S_c;
    m->gd_last_Sn = S_n;
    if (S_out) *S_out = S_c;
    if (logits_last) {
        HIPCHK(hipMemcpyAsync(logits_last, m->logits.p, (size_t)2 * B * m->c.vocab * 4, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
    }
}

// whether the pending vc_request_speculation is served by a call of this form (the LDS bound of the verify attention is known
// behind the prefill only): greedy and no processors — or any selection, with vc_request_speculation_selection — the bf16 step,
// B * (k + 1) rows in one weight pass
bool spec_request_served(const vc_model* m, const GenParams& g, int B) {
    return m->spec_k > 0 && !g.cn && (m->spec_any || (!g.do_sample && !g.proc)) && m->precision == 0 && B * (m->spec_k + 1) <= SPEC_MAX_ROWS;
}

// generate() on the session's own loop: prefill, then max_new - 1 graph-replayed (strict: eagerly enqueued) decode steps — or, with a
// served speculation request, verify steps until every row is finished or full.
// fan > 1 (a served vc_request_fanout): the B prompts are prefilled once, into rows 0 .. B - 1 of a cache of R = B fan rows; the loop
// runs over the R rows b fan + j, whose step 0 reads prompt b's logits row and whose steps attend with the fan-out kernel — prompt
// keys from cache row b, own keys from cache row b fan + j (positions >= S: the two regions of a cache row never overlap).  ids,
// log-probs and the callback's columns are R rows wide; the session's loop is closed behind the call.
// gd != nullptr (a served vc_request_guidance; fan == 1): the loop runs over Rs = 2 B rows — the B rows of the call, whose ids,
// log-probs and callback columns come back as ever, and their B followers behind the negative prompt (prefill_guided_on_session) —
// with the guided selection tail (LoopView::gd_logits); the session's loop is closed behind the call.
void generate_on_session(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                         int on_dev, const GenParams& g, const std::vector<int>& tail, vc_token_cb cb, void* cb_user,
                         int cb_every, int32_t* out_ids, int* n_generated, int fan = 1, const GuidanceCall* gd = nullptr) {
    const int max_new = g.max_new;
    const int R = B * fan;   // rows of the loop that return ids
    const int Rs = gd ? 2 * B : R;   // rows of a step
    m->spec_closed = false;
    m->fan_closed = false;
    m->gd_closed = false;
    int S_neg = 0;
    std::unique_lock<std::mutex> gate;
    if (gd) {
        gate = prefill_guided_on_session(m, *gd, ids, B, T, img, seg, depth, on_dev, 1, max_new, false, nullptr, &S_neg);   // generate() always builds a mask
    } else {
        m->fan_rows = fan > 1 ? R : 0;   // the prefill sizes the cache and the loop's buffers for R rows
        gate = prefill_on_session(m, ids, B, T, img, seg, depth, on_dev, max_new);
        m->fan_rows = 0;
    }
    ensure_out_ids(m, R, max_new);
    // vc_request_speculation: served when the call's form allows (spec_request_served) and the score rows of Q queries over this
    // cache fit a CU's LDS.  (A row drafts no further than its last slot, so the prefill's reserve of max_new positions holds.)
    const int Q = fan == 1 && !gd && spec_request_served(m, g, B) ? m->spec_k + 1 : 0;
    const bool spec = Q > 0 && (m->hd == 128 || m->hd == 64) && (m->kv_es == 2 || m->kv_es == 1) &&
                      attention_verify_lds_bytes(Q, m->hd, m->kv_es == 1, m->capS) <= ATTN_VERIFY_LDS_MAX;
    // the steps of this call: the session's plain view, plus what the call asked for — the view goes to the step-0 selection, to the
    // captured step (STEP_CALL with either request, else the plain one) and, in strict mode, to the eager step
    LoopView v = session_view(m);
    // vc_request_generate_logprobs: every selection of this call is followed by the log-prob launch
    const bool want_lp = m->glp_tok != nullptr;
    const int K = m->glp_k;
    if (want_lp) {
        ensure_logprob_slabs(m, R, K);
        v.lp_tok = m->lp_tok.as<float>();
        v.lp_top = m->lp_top.as<float>();
        v.lp_ids = m->lp_ids.as<int>();
        v.lp_k = K;
        // positions nothing writes (behind max_new, or never reached) read 0.0 / 0.0 / -1
        HIPCHK(hipMemsetAsync(m->lp_tok.p, 0, m->lp_tok.cap, m->st));
        HIPCHK(hipMemsetAsync(m->lp_top.p, 0, m->lp_top.cap, m->st));
        HIPCHK(hipMemsetAsync(m->lp_ids.p, 0xFF, m->lp_ids.cap, m->st));
    }
    // vc_request_logits_processors: every selection of this call is preceded by the processor launch, which reads the caller's
    // prompt ids (as int32, placeholders and all) and the bad-word table
    std::vector<int> ids32;
    if (g.proc) {
        ensure_processor_buffers(m, R, T);
        ids32.resize((size_t)B * T);
        for (size_t i = 0; i < ids32.size(); ++i) ids32[i] = (int)std::max<int64_t>(std::min<int64_t>(ids[i], INT32_MAX), INT32_MIN);
        HIPCHK(hipMemcpyAsync(m->proc_prompt.p, ids32.data(), ids32.size() * 4, hipMemcpyHostToDevice, m->st));
        if (!m->gproc_bad.empty())   // (a call with a token automaton alone brings no table: RS_LP_NBAD is 0)
            HIPCHK(hipMemcpyAsync(m->proc_bad.p, m->gproc_bad.data(), m->gproc_bad.size() * 4, hipMemcpyHostToDevice, m->st));
        // (both host vectors live until the synchronize behind the step-0 selection)
        v.proc_prompt = m->proc_prompt.as<int>();
        v.proc_bad = m->proc_bad.as<int>();
        v.proc_logits = m->proc_logits.as<float>();
    }
    // vc_request_constraint: the processor launch masks the processed rows by the rows' automaton states (RS_CN_*)
    if (g.cn) {
        const size_t S = (size_t)m->gcn_S, E = (size_t)m->gcn_E;
        REQUIRE(g.proc && m->gcn_tab.size() == 2 * S + 1 + 2 * E, VC_ERR_STATE, "token automaton tables of %zu ints", m->gcn_tab.size());
        m->cn_tab.ensure(m->gcn_tab.size() * 4);
        HIPCHK(hipMemcpyAsync(m->cn_tab.p, m->gcn_tab.data(), m->gcn_tab.size() * 4, hipMemcpyHostToDevice, m->st));   // (lives as above)
        v.cn_state_off = m->cn_tab.as<int>();
        v.cn_edge_tok = v.cn_state_off + S + 1;
        v.cn_edge_next = v.cn_edge_tok + E;
        v.cn_default_next = v.cn_edge_next + E;
        v.cn_states = m->gcn_S;
    }
    // the stop-sequence tails of the loop's rows on the host (row r: prompt r / fan)
    std::vector<int> tail_rows;
    if (fan > 1) {
        constexpr int TL = VC_MAX_STOP_LEN - 1;
        tail_rows.resize((size_t)R * TL);
        for (int r = 0; r < R; ++r) std::copy(tail.begin() + (size_t)(r / fan) * TL, tail.begin() + (size_t)(r / fan + 1) * TL, tail_rows.begin() + (size_t)r * TL);
    }
    const std::vector<int>& tails = fan > 1 ? tail_rows : tail;
    std::vector<int> fan_len(VC_MAX_ROWS, m->last_S);   // every group's prompt length (lives until the synchronize below)
    if (fan > 1) {
        m->fan_P.ensure(fan_len.size() * 4);
        HIPCHK(hipMemcpyAsync(m->fan_P.p, fan_len.data(), fan_len.size() * 4, hipMemcpyHostToDevice, m->st));
        v.fan_n = fan;
        v.fan_P = m->fan_P.as<int>();
    }
    if (gd) {
        m->gd_logits.ensure((size_t)rup(B, 16) * m->c.vocab * 4);
        m->gd_scalars.ensure((size_t)VC_MAX_ROWS * 4 * 4);
        v.gd_logits = m->gd_logits.as<float>();
        v.gd_scalars = m->gd_scalars.as<float>();
        arm_guided_rows(m, g, tail.data(), B, m->last_S, S_neg, gd->scale);
    } else {
        arm_session_rows(m, g, tail.data(), fan);
    }
    // token 0 comes from the prefill logits
    std::vector<int> fill((size_t)R * m->out_stride, g.pad);
    HIPCHK(hipMemcpyAsync(m->out_ids.p, fill.data(), fill.size() * 4, hipMemcpyHostToDevice, m->st));
    if (fan > 1) {
        // row r selects from prompt r / fan's logits row: the rows spread in place, last first (a source row r / fan <= r is only
        // overwritten by the copy for row r / fan itself, which comes later)
        const size_t rowb = (size_t)m->c.vocab * 4;
        for (int r = R - 1; r >= 1; --r)
            if (r / fan != r)
                HIPCHK(hipMemcpyAsync(reinterpret_cast<char*>(v.logits) + r * rowb, reinterpret_cast<char*>(v.logits) + (r / fan) * rowb, rowb,
                                      hipMemcpyDeviceToDevice, m->st));
    }
    enqueue_selection(m, v, v.logits, Rs, 1);   // step 0 -> 1; the position stays at S
    HIPCHK(hipStreamSynchronize(m->st));
    gate.unlock();
    int produced = 1, reported = 0;
    const bool can_finish = g.eos >= 0 || g.n_stop > 0;
    std::vector<int> rec((size_t)R * RS_STRIDE), part;
    auto all_finished = [&]() {
        if (!can_finish) return false;
        HIPCHK(hipMemcpyAsync(rec.data(), m->rows.p, rec.size() * 4, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        for (int b = 0; b < R; ++b)
            if (!rec[(size_t)b * RS_STRIDE + RS_FINISHED]) return false;
        return true;
    };
    auto report = [&](int upto) {  // streamer callback: columns [reported, upto) of every row
        if (!cb || upto <= reported) return;
        part.resize((size_t)R * (upto - reported));
        HIPCHK(hipMemcpy2DAsync(part.data(), (size_t)(upto - reported) * 4, m->out_ids.as<int>() + reported,
                                (size_t)m->out_stride * 4, (size_t)(upto - reported) * 4, R, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        cb(cb_user, reported, upto - reported, R, part.data());
        reported = upto;
    };
    const int every = cb ? std::max(cb_every, 1) : 8;
    if (cb && every == 1) report(1);
    if (spec) {
        // the verify loop: every replay emits 1 .. Q tokens per row, so a row's progress is its record's, not the host's step count
        const bool any = m->spec_any;
        ensure_spec(m, B * Q, any, g.proc != 0);
        const int ld = m->c.max_positions;
        const bool lookup = !m->spec_lookup.empty();
        std::vector<int> ids32((size_t)B * T), st(SPEC_STATE_INTS, 0);
        for (size_t i = 0; i < ids32.size(); ++i) ids32[i] = (int)std::max<int64_t>(std::min<int64_t>(ids[i], INT32_MAX), INT32_MIN);
        for (int b = 0; b < B; ++b) {
            st[5 * VC_MAX_ROWS + b] = T;
            st[6 * VC_MAX_ROWS + b] = lookup ? m->spec_lookup_len[b] : 0;
        }
        REQUIRE(T <= ld, VC_ERR_INVALID, "prompt of %d ids exceeds max_position_embeddings=%d", T, ld);
        HIPCHK(hipMemcpy2DAsync(m->sp_prompt.p, (size_t)ld * 4, ids32.data(), (size_t)T * 4, (size_t)T * 4, B, hipMemcpyHostToDevice, m->st));
        if (lookup && m->spec_lookup_stride > 0)
            HIPCHK(hipMemcpy2DAsync(m->sp_lookup.p, (size_t)ld * 4, m->spec_lookup.data(), (size_t)m->spec_lookup_stride * 4,
                                    (size_t)m->spec_lookup_stride * 4, B, hipMemcpyHostToDevice, m->st));
        HIPCHK(hipMemcpyAsync(m->sp_state.p, st.data(), st.size() * 4, hipMemcpyHostToDevice, m->st));
        HIPCHK(hipStreamSynchronize(m->st));   // the host vectors
        const SpecLoop sl = spec_view(m, B, Q, m->spec_ngram, lookup, want_lp ? K : -1, any, g.proc != 0);
        const LoopView sv = spec_loop_view(m, v);
        // -> every row finished or full; least tokens an unfinished row still has to emit; least step over the unfinished rows
        int left = 0, low = 0;
        auto poll = [&]() {
            HIPCHK(hipMemcpyAsync(rec.data(), m->rows.p, rec.size() * 4, hipMemcpyDeviceToHost, m->st));
            HIPCHK(hipStreamSynchronize(m->st));
            left = 0;
            low = max_new;
            produced = 0;
            for (int b = 0; b < B; ++b) {
                const int* r = rec.data() + (size_t)b * RS_STRIDE;
                produced = std::max(produced, std::min(r[RS_STEP], max_new));
                if (r[RS_FINISHED] || r[RS_STEP] >= max_new) continue;
                left = std::max(left, max_new - r[RS_STEP]);
                low = std::min(low, r[RS_STEP]);
            }
            return left == 0;
        };
        if (max_new > 1 && !poll()) {
            const hipGraphExec_t exec = spec_step_graph(m, sv, sl);
            do {
                // that many steps are needed whatever is accepted; a row that may finish early, or a streamer, is looked at sooner
                int n = std::max(1, (left + Q - 1) / Q);
                if (can_finish || cb) n = std::min(n, every);
                for (int i = 0; i < n; ++i) HIPCHK(hipGraphLaunch(exec, m->st));
                const bool done = poll();
                if (cb) report(done ? produced : low);
                if (done) break;
            } while (true);
        }
        m->spec_counters.assign((size_t)B * 4, 0);
        HIPCHK(hipMemcpyAsync(m->spec_counters.data(), sl.counters, (size_t)B * 16, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        m->spec_last = true;
        m->cur_pos = -1;       // the rows stand at different positions: the session's loop is closed
        m->spec_closed = true;
    } else if (max_new > 1 && !all_finished()) {
        const StepKind kind = gd ? STEP_GUIDE : (fan > 1 ? STEP_FAN : (want_lp || g.proc ? STEP_CALL : STEP_PLAIN));
        const hipGraphExec_t exec = m->precision != 1 ? step_graph(m, kind, v, Rs) : nullptr;
        for (int step = 1; step < max_new; ++step) {
            if (m->precision == 1) enqueue_decode_step_strict(m, v, B);
            else HIPCHK(hipGraphLaunch(exec, m->st));
            m->cur_pos += 1;
            produced = step + 1;
            // the reference checks its stopping criteria on the host every token; checking every few tokens only
            // trims later (rows past EOS already emit pad), it never changes the returned ids
            if ((step + 1) % every == 0 || step == max_new - 1) {
                if (cb) report(produced);
                if (can_finish) {
                    HIPCHK(hipStreamSynchronize(m->st));
                    if (all_finished()) break;
                }
            }
        }
    }
    if (m->ev[3]) HIPCHK(hipEventRecord(m->ev[3], m->st));
    HIPCHK(hipMemcpy2DAsync(out_ids, (size_t)max_new * 4, m->out_ids.p, (size_t)m->out_stride * 4, (size_t)max_new * 4, R,
                            hipMemcpyDeviceToHost, m->st));
    if (want_lp) {   // the slabs come back once, beside out_ids
        HIPCHK(hipMemcpy2DAsync(m->glp_tok, (size_t)max_new * 4, m->lp_tok.p, (size_t)m->out_stride * 4, (size_t)max_new * 4, R,
                                hipMemcpyDeviceToHost, m->st));
        if (K > 0) {
            HIPCHK(hipMemcpy2DAsync(m->glp_top, (size_t)max_new * K * 4, m->lp_top.p, (size_t)m->out_stride * K * 4,
                                    (size_t)max_new * K * 4, R, hipMemcpyDeviceToHost, m->st));
            HIPCHK(hipMemcpy2DAsync(m->glp_ids, (size_t)max_new * K * 4, m->lp_ids.p, (size_t)m->out_stride * K * 4,
                                    (size_t)max_new * K * 4, R, hipMemcpyDeviceToHost, m->st));
        }
    }
    HIPCHK(hipStreamSynchronize(m->st));
    if (want_lp) {
        // a row's finishing token (its EOS, or the token completing a stop sequence) is scored; behind it the row emitted pad: those
        // positions, and the columns the loop never reached, hold 0.0 / 0.0 / -1
        for (int b = 0; b < R; ++b) {
            const int e = row_finish_end(g, out_ids + (size_t)b * max_new, tails.data() + (size_t)b * (VC_MAX_STOP_LEN - 1), produced);
            for (int s_ = e; s_ < max_new; ++s_) {
                const size_t i = (size_t)b * max_new + s_;
                m->glp_tok[i] = 0.f;
                for (int k = 0; k < K; ++k) {
                    m->glp_top[i * K + k] = 0.f;
                    m->glp_ids[i * K + k] = -1;
                }
            }
        }
    }
    produced = trim_columns(g, out_ids, max_new, tails.data(), R, produced);
    if (cb) report(produced);
    if (fan > 1) {
        m->cur_pos = -1;       // cache row r holds prompt r's keys and sequence r's own: the session's loop is closed
        m->fan_closed = true;
    }
    if (gd) {
        m->cur_pos = -1;       // the conditional rows and their followers stand at different positions: the session's loop is closed
        m->gd_closed = true;
        m->gd_last = true;     // (set behind the loop: a call that failed reports no served request)
        m->gd_last_B = B;
        m->gd_last_Sc = m->last_S;
        m->gd_last_Sn = S_neg;
    }
    if (n_generated) *n_generated = produced;
    read_phase_times(m, m->ev[2], m->ev[3]);
}

// ---- beam search inside the device loop (vc_generate_beam) -----------------------------------------------------------------------
struct BeamCall {
    int n = 1, max_new = 1, n_eos = 0, pad = -1, early = 0, len_counts_prompt = 1;
    float length_penalty = 1.f;
    int eos[VC_BEAM_MAX_EOS] = {};
};
struct BeamHypHost {
    float score, sum;
    int step, row;
};
// BeamHypotheses.add on the host, as beam_step_kernel states it (fp32; the worst — the first of equals — leaves, order kept)
void beam_add_hyp(std::vector<BeamHypHost>& list, float& worst, int n, float sum, float den, int step, int row) {
    const float score = sum / den;
    if ((int)list.size() >= n && !(score > worst)) return;
    if ((int)list.size() >= n) {
        size_t lo = 0;
        for (size_t j = 1; j < list.size(); ++j)
            if (list[j].score < list[lo].score) lo = j;
        list.erase(list.begin() + lo);
    }
    list.push_back({score, sum, step, row});
    worst = score;
    for (const BeamHypHost& h : list) worst = std::min(worst, h.score);
}

// Every sequence expanded to n rows (rows b * n .. b * n + n - 1, as HF's _expand_inputs_for_generation) for the encode, the splice
// and the prefill; then one eager beam tail on the prefill logits and max_new - 1 replays of the captured beam step, polled every
// 8 steps for "every sequence done"; the tables, hypotheses, beam scores and sequence records come back once and the tail of HF's
// beam_search (BeamSearchScorer.finalize) runs here in fp32.
void generate_beam_on_session(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                              int on_dev, const BeamCall& q, int32_t* out_ids, int32_t* out_len, float* out_score, int* n_steps) {
    const vc_model_cfg& c = m->c;
    const int n = q.n, R = B * n, max_new = q.max_new;
    std::vector<int64_t> ids_x((size_t)R * T);
    for (int r = 0; r < R; ++r) std::copy(ids + (size_t)(r / n) * T, ids + (size_t)(r / n + 1) * T, ids_x.begin() + (size_t)r * T);
    if (!m->mask_next.empty()) {
        REQUIRE(m->mask_B == B && m->mask_T == T, VC_ERR_INVALID, "attention_mask is [%d, %d], input_ids [%d, %d]", m->mask_B, m->mask_T,
                B, T);
        std::vector<uint8_t> mk((size_t)R * T);
        for (int r = 0; r < R; ++r)
            std::copy(m->mask_next.begin() + (size_t)(r / n) * T, m->mask_next.begin() + (size_t)(r / n + 1) * T, mk.begin() + (size_t)r * T);
        m->mask_next.swap(mk);
        m->mask_B = R;
    }
    // pixels: the images of sample b (img_counts, one each without them) n times in a row
    const float* src[3] = {img, img ? seg : nullptr, img ? depth : nullptr};
    const size_t img_elems = (size_t)3 * c.vit_image * c.vit_image;
    std::vector<float> host_px[3];
    Buf dev_px[3];
    struct Release {
        Buf* b;
        ~Release() {
            for (int k = 0; k < 3; ++k) b[k].release();
        }
    } release{dev_px};
    const float* px[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) {
        if (!src[k]) continue;
        std::vector<int> cnt = m->img_counts[k];
        if (cnt.empty()) cnt.assign(B, 1);
        REQUIRE((int)cnt.size() == B, VC_ERR_INVALID, "image counts given for %zu samples, batch is %d", cnt.size(), B);
        size_t total = 0;
        for (int b = 0; b < B; ++b) total += (size_t)cnt[b] * n;
        if (on_dev) dev_px[k].ensure(total * img_elems * 4);
        else host_px[k].resize(total * img_elems);
        float* dst = on_dev ? dev_px[k].as<float>() : host_px[k].data();
        size_t first = 0, at = 0;
        for (int b = 0; b < B; ++b) {
            const size_t blk = (size_t)cnt[b] * img_elems;
            for (int j = 0; j < n; ++j, at += blk) {
                if (on_dev) HIPCHK(hipMemcpyAsync(dst + at, src[k] + first, blk * 4, hipMemcpyDeviceToDevice, m->st));
                else std::copy(src[k] + first, src[k] + first + blk, dst + at);
            }
            first += blk;
        }
        if (!m->img_counts[k].empty()) {
            std::vector<int> cx;
            for (int b = 0; b < B; ++b) cx.insert(cx.end(), n, cnt[b]);
            m->img_counts[k].swap(cx);
        }
        px[k] = dst;
    }
    std::unique_lock<std::mutex> gate = prefill_on_session(m, ids_x.data(), R, T, px[0], px[1], px[2], on_dev, max_new);
    const int S = m->last_S;
    ensure_beam(m, R, max_new);
    // the tail permute cuts a tail at the span its grid and staging are sized for: the whole call must fit (it does: cap_new >= max_new)
    REQUIRE(max_new <= m->bm_cap_new && m->bm_tmp.cap >= (size_t)2 * R * c.heads * beam_span_cap(m, m->bm_cap_new), VC_ERR_STATE,
            "beam buffers hold %d steps, the call asks for %d", m->bm_cap_new, max_new);
    GenParams none;   // nothing is recorded in out_ids, no EOS bookkeeping in the records: the beam kernel keeps its own
    arm_session_rows(m, none, nullptr);
    const LoopView v = session_view(m);
    const BeamLoop bl = beam_view(m, B, n);
    // the state of step 0: beam 0 of every sequence alive, the others at -1e9 (HF: beam_scores[:, 1:] = -1e9), no hypotheses
    int* const base = m->bm_state.as<int>();
    std::vector<int> st(BEAM_STATE_INTS, 0);
    auto at = [&](const void* p) { return st.data() + (reinterpret_cast<const int*>(p) - base); };
    const float worst0 = 1e9f;
    for (int r = 0; r < R; ++r) {
        const float s0 = r % n ? -1e9f : 0.f;
        memcpy(at(bl.score) + r, &s0, 4);
        at(bl.perm)[r] = r;
        at(bl.start)[r] = S;
    }
    for (int b = 0; b < B; ++b) memcpy(at(bl.seq) + b * BQ_STRIDE + BQ_WORST, &worst0, 4);
    int* prm = at(bl.params);
    prm[BP_N_EOS] = q.n_eos;
    prm[BP_PAD] = q.pad >= 0 ? q.pad : 0;
    prm[BP_EARLY] = q.early;
    prm[BP_MAXNEW] = max_new;
    for (int e = 0; e < q.n_eos; ++e) prm[BP_EOS + e] = q.eos[e];
    // the two denominator tables (no powf on the device): hypothesis length -> length ** length_penalty, in double as the host loop
    auto hyp_len = [&](int len) { return q.len_counts_prompt ? len : len - T; };
    auto den_of = [&](int hl) { return (float)std::pow((double)std::max(hl, 1), (double)q.length_penalty); };
    std::vector<float> den((size_t)2 * (bl.cap_new + 1), 1.f);
    for (int s_ = 0; s_ <= max_new; ++s_) {
        den[s_] = den_of(hyp_len(T + s_));
        den[bl.cap_new + 1 + s_] = q.early == 2 && q.length_penalty > 0.f ? den_of(hyp_len(T + max_new)) : den[s_];
    }
    HIPCHK(hipMemcpyAsync(base, st.data(), st.size() * 4, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(m->bm_den.p, den.data(), den.size() * 4, hipMemcpyHostToDevice, m->st));
    enqueue_beam_tail(m, v, bl, v.logits, 1, false);   // step 0 -> 1 on the prefill logits; the position stays at S
    HIPCHK(hipStreamSynchronize(m->st));   // (`st`, `den` are host memory)
    gate.unlock();
    int fl[2] = {0, 0};
    auto poll = [&]() {
        HIPCHK(hipMemcpyAsync(fl, bl.flags, 8, hipMemcpyDeviceToHost, m->st));
        HIPCHK(hipStreamSynchronize(m->st));
        return fl[0] || fl[1];
    };
    int produced = 1;
    if (!poll() && max_new > 1) {
        const hipGraphExec_t exec = step_graph(m, STEP_BEAM, v, R, &bl);
        for (int step = 1; step < max_new; ++step) {
            HIPCHK(hipGraphLaunch(exec, m->st));
            m->cur_pos += 1;
            produced = step + 1;
            // a done sequence emits pad and changes nothing: polling every few steps only ends the loop later
            if (((step + 1) % 8 == 0 || step == max_new - 1) && poll()) break;
        }
    }
    if (m->ev[3]) HIPCHK(hipEventRecord(m->ev[3], m->st));
    std::vector<int> tok((size_t)produced * R), par((size_t)produced * R);
    HIPCHK(hipMemcpyAsync(st.data(), base, st.size() * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipMemcpyAsync(tok.data(), bl.tok_tab, tok.size() * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipMemcpyAsync(par.data(), bl.parent_tab, par.size() * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    REQUIRE(!at(bl.flags)[1], VC_ERR_INVALID, "At most %d tokens among the %d best continuations of a sequence can be equal to `eos_token_id: %d`.",
            n, 2 * n, q.n_eos ? q.eos[0] : -1);
    // steps the host loop would have run: up to the step that finished the last sequence, or all of them
    bool all_done = true;
    int steps = 0;
    for (int b = 0; b < B; ++b) {
        all_done = all_done && at(bl.seq)[b * BQ_STRIDE + BQ_DONE];
        steps = std::max(steps, at(bl.seq)[b * BQ_STRIDE + BQ_DONE_STEP] + 1);
    }
    if (!all_done) steps = produced;
    if (n_steps) *n_steps = steps;
    // finalize: open beams of unfinished sequences become hypotheses, the best one (the first of equals) is returned
    std::vector<std::vector<int>> best_ids(B);
    int L = 0;
    for (int b = 0; b < B; ++b) {
        const int* sq = at(bl.seq) + b * BQ_STRIDE;
        std::vector<BeamHypHost> list;
        for (int j = 0; j < sq[BQ_NHYP]; ++j) {
            const int* h = at(bl.hyp) + ((size_t)b * n + j) * BH_STRIDE;
            BeamHypHost e;
            memcpy(&e.score, h + BH_SCORE, 4);
            memcpy(&e.sum, h + BH_SUM, 4);
            e.step = h[BH_STEP];
            e.row = h[BH_ROW];
            list.push_back(e);
        }
        float worst;
        memcpy(&worst, sq + BQ_WORST, 4);
        if (!sq[BQ_DONE])
            for (int j = 0; j < n; ++j) {
                float sum;
                memcpy(&sum, at(bl.score) + b * n + j, 4);
                beam_add_hyp(list, worst, n, sum, den[steps], steps, b * n + j);
            }
        size_t bi = 0;
        for (size_t j = 1; j < list.size(); ++j)
            if (list[j].score > list[bi].score) bi = j;
        const BeamHypHost& h = list[bi];
        REQUIRE(h.step >= 0 && h.step <= produced && h.row >= 0 && h.row < R, VC_ERR_STATE, "beam hypothesis (%d, %d) outside the tables",
                h.step, h.row);
        std::vector<int>& out = best_ids[b];
        out.resize(h.step);
        for (int s_ = h.step - 1, r = h.row; s_ >= 0; --s_) {   // back-pointers: the token of row r at step s_, then its parent
            out[s_] = tok[(size_t)s_ * R + r];
            r = par[(size_t)s_ * R + r];
        }
        out_len[b] = h.step;
        out_score[b] = h.score;
        L = std::max(L, h.step);
    }
    const int L_out = std::min(L + 1, max_new);   // BeamSearchScorer.finalize: room for the EOS a finished hypothesis does not carry
    for (int b = 0; b < B; ++b)
        REQUIRE((int)best_ids[b].size() >= L_out || q.pad >= 0, VC_ERR_INVALID, "`pad_token_id` has to be defined");
    for (int b = 0; b < B; ++b) {
        int32_t* row = out_ids + (size_t)b * max_new;
        std::fill(row, row + max_new, q.pad >= 0 ? q.pad : 0);
        std::copy(best_ids[b].begin(), best_ids[b].end(), row);
        if ((int)best_ids[b].size() < L_out && q.n_eos > 0) row[best_ids[b].size()] = q.eos[0];
    }
    read_phase_times(m, m->ev[2], m->ev[3]);
}

// Whether one prefill of a prompt yields the bits every one of its `fan` copies gets in the repeated call — what the fan-out form rests
// on, since the repeated call defines the result.  The prefill's rows are independent of what shares their launch except in the GEMMs'
// split-K remainder round (attach_splitk_ws: its k-slices depend on the tile a row falls into, so identical prompts of one batch may
// even differ among themselves).  True in the batch-invariant mode, which has no such round, and when no GEMM of the REPEATED call's
// encode + prefill can have more than one round of 256 x 256 tiles: then none gets the workspace either.  The spliced length is not
// known yet: the rows are bounded as generate_on_pool bounds them, and the widest GEMM is paired with the longest.
bool fanout_prefill_bits_shared(const vc_model* m, int B, int T, int fan) {
    if (batch_invariant(m)) return true;
    const vc_model_cfg& c = m->c;
    long images = 0, per_sample = 3;
    for (int k = 0; k < 3; ++k) {
        const std::vector<int>& cnt = m->img_counts[k];
        long n_k = B;
        if ((int)cnt.size() == B) {
            n_k = 0;
            for (int b = 0; b < B; ++b) n_k += cnt[b];
        }
        images += n_k;
    }
    for (int b = 0; b < B; ++b) {
        long n_b = 0;
        for (int k = 0; k < 3; ++k) n_b += (int)m->img_counts[k].size() == B ? m->img_counts[k][b] : 1;
        per_sample = std::max(per_sample, n_b);
    }
    const long S_bound = std::min<long>(c.max_positions, T + per_sample * m->Tv);
    const long rows = std::max<long>((long)B * fan * (long)rup((size_t)S_bound, 32), images * fan * m->Tv);
    const long wide = std::max({3L * c.hidden, 2L * c.ffn, 3L * c.vit_hidden, (long)c.vit_ffn});
    return ((rows + 255) / 256) * ((wide + 255) / 256) <= 256;
}

// a fan-out request that is not served: the call's inputs with every prompt repeated fan times (HF's _expand_inputs_for_generation)
struct FanExpanded {
    std::vector<int64_t> ids;
    std::vector<float> host_px[3];
    const float* px[3] = {nullptr, nullptr, nullptr};
    std::vector<int> tail;
};
FanExpanded expand_for_fanout(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                              int on_dev, int fan, const std::vector<int>& tail) {
    FanExpanded x;
    const int R = B * fan;
    constexpr int TL = VC_MAX_STOP_LEN - 1;
    x.ids.resize((size_t)R * T);
    x.tail.resize((size_t)R * TL);
    for (int r = 0; r < R; ++r) {
        std::copy(ids + (size_t)(r / fan) * T, ids + (size_t)(r / fan + 1) * T, x.ids.begin() + (size_t)r * T);
        std::copy(tail.begin() + (size_t)(r / fan) * TL, tail.begin() + (size_t)(r / fan + 1) * TL, x.tail.begin() + (size_t)r * TL);
    }
    const size_t img_elems = (size_t)3 * m->c.vit_image * m->c.vit_image;
    const float* src[3] = {img, seg, depth};
    for (int k = 0; k < 3; ++k) {
        if (!src[k]) continue;
        std::vector<int>& cnt = m->img_counts[k];
        REQUIRE(cnt.empty() || (int)cnt.size() == B, VC_ERR_INVALID, "image counts given for %zu samples, batch is %d", cnt.size(), B);
        std::vector<size_t> first(B + 1, 0);   // first image of every sample
        for (int b = 0; b < B; ++b) first[b + 1] = first[b] + (cnt.empty() ? 1 : cnt[b]);
        const size_t total = first[B] * fan * img_elems;
        float* dst = nullptr;
        if (on_dev) {
            m->fan_px[k].ensure(std::max<size_t>(total, 1) * 4);
            dst = m->fan_px[k].as<float>();
        } else {
            x.host_px[k].resize(total);
            dst = x.host_px[k].data();
        }
        size_t at = 0;
        for (int r = 0; r < R; ++r) {
            const int b = r / fan;
            const size_t n = (first[b + 1] - first[b]) * img_elems;
            if (on_dev) HIPCHK(hipMemcpyAsync(dst + at, src[k] + first[b] * img_elems, n * 4, hipMemcpyDeviceToDevice, m->st));
            else std::copy(src[k] + first[b] * img_elems, src[k] + first[b] * img_elems + n, dst + at);
            at += n;
        }
        x.px[k] = dst;
        if (!cnt.empty()) {
            std::vector<int> c2((size_t)R);
            for (int r = 0; r < R; ++r) c2[r] = cnt[r / fan];
            cnt.swap(c2);
        }
    }
    if (on_dev) HIPCHK(hipStreamSynchronize(m->st));
    if (!m->mask_next.empty()) {
        REQUIRE(m->mask_B == B && m->mask_T == T, VC_ERR_INVALID, "attention_mask is [%d, %d], input_ids [%d, %d]", m->mask_B, m->mask_T, B, T);
        std::vector<uint8_t> mk((size_t)R * T);
        for (int r = 0; r < R; ++r) std::copy(m->mask_next.begin() + (size_t)(r / fan) * T, m->mask_next.begin() + (size_t)(r / fan + 1) * T, mk.begin() + (size_t)r * T);
        m->mask_next.swap(mk);
        m->mask_B = R;
    }
    if (m->spec_k > 0 && !m->spec_lookup.empty()) {
        const size_t st = (size_t)std::max(m->spec_lookup_stride, 1);
        std::vector<int> lk((size_t)R * st), ln((size_t)R);
        for (int r = 0; r < R; ++r) {
            std::copy(m->spec_lookup.begin() + (size_t)(r / fan) * st, m->spec_lookup.begin() + (size_t)(r / fan + 1) * st, lk.begin() + (size_t)r * st);
            ln[r] = m->spec_lookup_len[r / fan];
        }
        m->spec_lookup.swap(lk);
        m->spec_lookup_len.swap(ln);
        m->spec_B = R;
    }
    return x;
}

}  // namespace

/* generate(): encode + splice + prefill + (max_new - 1) decode steps with the token selection on the device — greedy
 * (samp NULL or do_sample 0) or temperature / top-k / top-p sampling — EOS / pad bookkeeping, device-side keyword stops
 * and an optional streamer callback.  See include/vcoder_hip.h. */
VC_API int vc_generate(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                       int pixels_on_device, int max_new, int eos_id, int pad_id, const int32_t* stop_ids,
                       const int32_t* stop_lens, int n_stop, const vc_sampling* samp, vc_token_cb cb, void* cb_user,
                       int cb_every, int32_t* out_ids, int* n_generated) {
    if (!m) return VC_ERR_INVALID;
    OneShotReset one_shot{m};
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    REQUIRE(max_new >= 1 && out_ids, VC_ERR_INVALID, "bad max_new/out_ids");
    // vc_request_fanout: n rows per prompt, out_ids / the log-prob buffers / the callback's columns B n rows wide
    const int fan = m->fan_n > 1 ? m->fan_n : 1;
    m->fan_last = false;
    REQUIRE(B >= 1 && (long long)B * fan <= VC_MAX_ROWS, VC_ERR_INVALID,
            "batch %d x num_return_sequences %d exceeds the %d rows a replica decodes at a time", B, fan, VC_MAX_ROWS);
    REQUIRE(n_stop >= 0 && n_stop <= VC_MAX_STOP && (n_stop == 0 || (stop_ids && stop_lens)), VC_ERR_INVALID,
            "at most %d stop sequences", VC_MAX_STOP);
    // finished rows are fed the pad token's embedding: it must be a real row of embed_tokens
    REQUIRE(!(eos_id >= 0 || n_stop > 0) || (pad_id >= 0 && pad_id < m->c.vocab), VC_ERR_INDEX,
            "pad_token_id %d is outside the vocabulary (%d)", pad_id, m->c.vocab);
    GenParams g;
    g.max_new = max_new;
    g.eos = eos_id;
    g.pad = pad_id;
    g.n_stop = n_stop;
    for (int i = 0, off = 0; i < n_stop; ++i) {
        REQUIRE(stop_lens[i] >= 1 && stop_lens[i] <= VC_MAX_STOP_LEN, VC_ERR_INVALID, "stop sequence %d: 1..%d ids", i,
                VC_MAX_STOP_LEN);
        g.stop[i][0] = stop_lens[i];
        for (int j = 0; j < stop_lens[i]; ++j) g.stop[i][1 + j] = stop_ids[off + j];
        off += stop_lens[i];
    }
    if (samp && samp->do_sample) {
        REQUIRE(samp->temperature > 0.f, VC_ERR_INVALID, "temperature must be positive (got %g)", (double)samp->temperature);
        REQUIRE(samp->top_p > 0.f && samp->top_p <= 1.f, VC_ERR_INVALID, "top_p must be in (0, 1] (got %g)", (double)samp->top_p);
        g.do_sample = 1;
        g.temperature = samp->temperature;
        g.top_k = samp->top_k;
        g.top_p = samp->top_p;
        g.seed = samp->seed;
        // vc_request_sampling_warpers: into the records (a greedy call applies no warper, as in HF)
        g.min_p = m->warp_min_p;
        g.typical_p = m->warp_typical;
        g.epsilon_cutoff = m->warp_eps;
        g.eta_cutoff = m->warp_eta;
    }
    constexpr int TL = VC_MAX_STOP_LEN - 1;
    std::vector<int> tail((size_t)B * TL, INT32_MIN);  // ids never equal INT32_MIN
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < TL && j < T; ++j) tail[(size_t)b * TL + TL - 1 - j] = (int)ids[(size_t)b * T + T - 1 - j];
    // concurrent generate() calls share their decode steps in the root model's pool (VC_POOL=0: every call on its own
    // loop); strict mode keeps fp32 caches of its own
    static const bool use_pool = !(getenv("VC_POOL") && atoi(getenv("VC_POOL")) == 0);
    // vc_request_generate_logprobs: the call runs on the session's own loop, whose steps carry the log-prob launch
    REQUIRE(!m->glp_tok || m->glp_cap >= (size_t)B * fan * max_new, VC_ERR_INVALID,
            "log-prob buffers hold %zu rows, the call yields [%d, %d]", m->glp_cap, B * fan, max_new);
    // vc_request_logits_processors: likewise (the pool's steps carry no processor launch)
    if (m->gproc) {
        REQUIRE(m->gproc_bad.size() == (size_t)VC_MAX_BAD_WORDS * (1 + VC_MAX_BAD_WORD_LEN), VC_ERR_STATE, "bad-word table of %zu ints",
                m->gproc_bad.size());
        g.proc = 1;
        g.proc_penalty = m->gproc_penalty;
        g.proc_ngram = m->gproc_ngram;
        g.proc_minnew = m->gproc_minnew;
        g.proc_nbad = m->gproc_nbad;
        g.proc_neos = m->gproc_neos;
        for (int e = 0; e < m->gproc_neos; ++e) g.proc_eos[e] = m->gproc_eos[e];
        g.proc_T = T;
    }
    // vc_request_constraint: likewise, and the processor launch is what applies it — also when no processor is on (the RS_LP_* slots
    // of such a call hold their off values).  A pending vc_request_speculation is not served beside it (spec_request_served)
    if (!m->gcn_tab.empty()) {
        g.proc = 1;
        g.proc_T = T;
        g.cn = 1;
    }
    // vc_request_speculation: a served request runs on the session's own loop (the pool's steps are plain ones)
    REQUIRE(m->spec_k == 0 || m->spec_lookup.empty() || m->spec_B == B, VC_ERR_INVALID, "lookup ids given for %d sequences, batch is %d",
            m->spec_B, B);
    m->spec_last = false;
    // vc_request_guidance: the call runs on the session's own loop over 2 B rows (the pool's steps carry no guided tail); a pending
    // vc_request_speculation is not served beside it
    m->gd_last = false;
    if (m->gd_on) {
        REQUIRE(fan == 1, VC_ERR_STATE, "a vc_request_guidance and a vc_request_fanout are pending: repeat the prompts instead");
        REQUIRE(m->precision == 0, VC_ERR_STATE, "guidance is served in the bf16 precision mode");
        // guidance_follow_kernel copies the x / xg rows in 16-byte chunks: D a multiple of 8 puts every row start on 16 bytes
        REQUIRE(m->c.hidden % 8 == 0, VC_ERR_STATE, "the guided step copies rows in 16-byte chunks: hidden_size %d is no multiple of 8", m->c.hidden);
        REQUIRE(m->gd_B == B, VC_ERR_INVALID, "negative prompts given for %d sequences, batch is %d", m->gd_B, B);
        REQUIRE(2 * B <= VC_MAX_ROWS, VC_ERR_INVALID, "a guided batch of %d needs %d rows: at most %d per GPU replica", B, 2 * B, VC_MAX_ROWS);
        const GuidanceCall gd = take_guidance(m);
        generate_on_session(m, ids, B, T, img, seg, depth, pixels_on_device, g, tail, cb, cb_user, cb_every, out_ids, n_generated, 1, &gd);
    } else if (fan > 1) {
        // served: the bf16 step over a bf16 or e4m3 cache, head dim 128 or 64, up to 8 rows per prompt, n score rows over the
        // longest cache this model can ask for within a CU's LDS (the capacity itself is known behind the prefill only), and a
        // prefill whose bits do not depend on the rows that share its launch (else no shared prefix equals the repeated call)
        const int es = m->precision == 0 ? step_kv_es(m) : 0;
        const bool served = m->fan_share && m->precision == 0 && (m->hd == 128 || m->hd == 64) && (es == 2 || es == 1) && fan <= 8 &&
                            attention_fanout_lds_bytes(fan, m->hd, es == 1, m->c.max_positions / 64 * 64) <= ATTN_VERIFY_LDS_MAX &&
                            fanout_prefill_bits_shared(m, B, T, fan);
        m->fan_last = true;
        m->fan_last_n = fan;
        m->fan_last_shared = served;
        m->fan_last_B = served ? B : B * fan;
        if (served) {
            generate_on_session(m, ids, B, T, img, seg, depth, pixels_on_device, g, tail, cb, cb_user, cb_every, out_ids, n_generated, fan);
        } else {
            // not served: the replicated call, which defines the result — every prompt's ids, images, image counts, mask row,
            // lookup ids and stop tail fan times (rows b fan + j), then the existing path over B fan rows
            FanExpanded x = expand_for_fanout(m, ids, B, T, img, seg, depth, pixels_on_device, fan, tail);
            g.proc_T = T;
            const int R = B * fan;
            if (use_pool && m->precision != 1 && !m->glp_tok && !g.proc && !spec_request_served(m, g, R))
                generate_on_pool(m, x.ids.data(), R, T, x.px[0], x.px[1], x.px[2], pixels_on_device, g, x.tail, cb, cb_user, cb_every, out_ids,
                                 n_generated);
            else
                generate_on_session(m, x.ids.data(), R, T, x.px[0], x.px[1], x.px[2], pixels_on_device, g, x.tail, cb, cb_user, cb_every,
                                    out_ids, n_generated);
        }
    } else if (use_pool && m->precision != 1 && !m->glp_tok && !g.proc && !spec_request_served(m, g, B))
        generate_on_pool(m, ids, B, T, img, seg, depth, pixels_on_device, g, tail, cb, cb_user, cb_every, out_ids, n_generated);
    else
        generate_on_session(m, ids, B, T, img, seg, depth, pixels_on_device, g, tail, cb, cb_user, cb_every, out_ids,
                            n_generated);
    GUARD_END(m->ctx)
}

/* generate(num_beams = n) inside the device loop: every sequence expanded to n rows, one captured beam step per token (top 2 n
 * log-probs per row, the selection / hypothesis bookkeeping kernel, the tail-only cache permute, the embedding), HF's
 * BeamSearchScorer.finalize on the host.  See include/vcoder_hip.h. */
VC_API int vc_generate_beam(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg, const float* depth,
                            int pixels_on_device, int num_beams, int max_new, const int32_t* eos_ids, int n_eos, int pad_id,
                            float length_penalty, int early_stopping, int len_counts_prompt, int32_t* out_ids, int32_t* out_len,
                            float* out_score, int* n_steps) {
    if (!m) return VC_ERR_INVALID;
    OneShotReset one_shot{m};
    GUARD_BEGIN
    USE_DEVICE(m->ctx);
    // every refusal comes before anything of the session is touched
    REQUIRE(ids && B >= 1 && T >= 1 && max_new >= 1 && out_ids && out_len && out_score, VC_ERR_INVALID, "bad ids / B / T / max_new / outputs");
    REQUIRE(num_beams >= 1, VC_ERR_INVALID, "num_beams must be at least 1 (got %d)", num_beams);
    REQUIRE((long long)B * num_beams <= VC_BEAM_MAX_ROWS, VC_ERR_INVALID, "batch %d x num_beams %d exceeds the %d rows a replica decodes at a time",
            B, num_beams, VC_BEAM_MAX_ROWS);
    REQUIRE(n_eos >= 0 && n_eos <= VC_BEAM_MAX_EOS && (n_eos == 0 || eos_ids), VC_ERR_INVALID, "at most %d EOS ids", VC_BEAM_MAX_EOS);
    REQUIRE(early_stopping >= 0 && early_stopping <= 2, VC_ERR_INVALID, "early_stopping: 0 (false), 1 (true) or 2 (\"never\")");
    REQUIRE(pad_id < m->c.vocab, VC_ERR_INDEX, "pad_token_id %d is outside the vocabulary (%d)", pad_id, m->c.vocab);
    REQUIRE(m->precision != 1, VC_ERR_STATE, "strict mode keeps beam search on the host loop (vc_decode_step + vc_reorder_cache)");
    REQUIRE(!m->glp_tok, VC_ERR_STATE, "per-token log-probs are not implemented for beam search: a vc_request_generate_logprobs is pending");
    REQUIRE(!m->gproc, VC_ERR_STATE, "logits processors are not implemented in the device beam loop: a vc_request_logits_processors is pending");
    REQUIRE(m->gcn_tab.empty(), VC_ERR_STATE, "constrained decoding is not implemented in the device beam loop: a vc_request_constraint is pending");
    REQUIRE(!m->gd_on, VC_ERR_STATE, "guidance is not implemented in the device beam loop: a vc_request_guidance is pending");
    m->spec_last = false;   // (a pending vc_request_speculation is not served by beam search)
    {   // the tail permute moves 16-byte chunks of a cache row: the element size the prefill below will give the session's cache
        const int es = m->precision == 2 ? split_kv_es() : step_kv_es(m);
        REQUIRE((m->hd * es) % 16 == 0, VC_ERR_STATE, "the tail permute moves 16-byte chunks: head_dim %d x %d bytes", m->hd, es);
    }
    BeamCall q;
    q.n = num_beams;
    q.max_new = max_new;
    q.n_eos = n_eos;
    for (int e = 0; e < n_eos; ++e) q.eos[e] = eos_ids[e];
    q.pad = pad_id;
    q.early = early_stopping;
    q.len_counts_prompt = len_counts_prompt != 0;
    q.length_penalty = length_penalty;
    generate_beam_on_session(m, ids, B, T, img, seg, depth, pixels_on_device, q, out_ids, out_len, out_score, n_steps);
    GUARD_END(m->ctx)
}

VC_API int vc_generate_greedy_stop(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                                   const float* depth, int pixels_on_device, int max_new, int eos_id, int pad_id,
                                   const int32_t* stop_ids, const int32_t* stop_lens, int n_stop, int32_t* out_ids,
                                   int* n_generated) {
    return vc_generate(m, ids, B, T, img, seg, depth, pixels_on_device, max_new, eos_id, pad_id, stop_ids, stop_lens, n_stop,
                       nullptr, nullptr, nullptr, 0, out_ids, n_generated);
}

/* spliced sequence length (text + feature rows) of the last vc_generate_greedy* call of this model / session */
VC_API int vc_last_spliced_len(vc_model* m) { return m ? m->last_S : VC_ERR_INVALID; }

VC_API int vc_generate_greedy(vc_model* m, const int64_t* ids, int B, int T, const float* img, const float* seg,
                              const float* depth, int pixels_on_device, int max_new, int eos_id, int pad_id,
                              int32_t* out_ids, int* n_generated) {
    return vc_generate_greedy_stop(m, ids, B, T, img, seg, depth, pixels_on_device, max_new, eos_id, pad_id, nullptr, nullptr,
                                   0, out_ids, n_generated);
}

// ---- image preprocessing: PIL's 8-bit bicubic coefficient tables (Pillow Resample.c: precompute_coeffs +
// normalize_coeffs_8bpc), built in double on the host ----------------------------------------------------------------
