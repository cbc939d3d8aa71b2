// select.hip — the tail of a decode step: token selection (greedy or sampled), EOS / keyword-stop bookkeeping, embedding
// of the selected token into the next step's residual stream and the per-row position advance — one workgroup per row.
//
//   greedy   : fp32 argmax, lowest index on ties            [HF] generation/utils.py:2894,2925
//   sampling : temperature -> top-k -> top-p -> multinomial  [HF] generation/logits_process.py (TemperatureLogitsWarper,
//              TopKLogitsWarper, TopPLogitsWarper) + utils.py:2921-2923; what vcoder_llava/serve/cli.py:122-132 asks for
//              (do_sample=True, temperature=0.2) and serve/chat.py:141-151 (temperature, top_p); behind top-p, when the row's
//              record asks for them: min-p -> typical -> epsilon -> eta (MinPLogitsWarper, TypicalLogitsWarper,
//              EpsilonLogitsWarper, EtaLogitsWarper; warp_thresholds below)
//   finished rows emit pad, EOS finishes a row                [HF] generation/utils.py:2928-2929
//   keyword stop: suffix match of the row's ids               vcoder_llava/mm_utils.py:128-151 (KeywordsStoppingCriteria)
//   embedding of the chosen token                             [HF] llama/modeling_llama.py:377
//   beam search: candidates, process, hypotheses, done        [HF] generation/utils.py beam_search, beam_search.py (4.31)
//
// Everything a row needs lives in its RowState record in device memory (kernels.h: RS_*), so ONE captured hipGraph serves
// every step of every request: rows of different requests (different prompt lengths, step counts, sampling parameters,
// stop sequences) can share a decode step.  Rows are independent; a row only ever touches its own record.
//
// Sampling runs entirely on the device: the scaled logits of the row sit in LDS (V * 4 bytes; 125 KiB for Llama's 32000),
// top-k and top-p thresholds are found by bit-wise bisection over the order-preserving integer image of the fp32 values
// (exact: 32 counting / mass passes over LDS, no sort), and the draw is a Gumbel-max over the kept set with a counter-based
// generator keyed by (seed, step, vocabulary index) — the same seed reproduces the same tokens, on any launch geometry.
#include "vc_device.h"
#include "kernels.h"

namespace vc {

VC_DEV void argmax_combine2(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// order-preserving map fp32 -> uint32 (negative values reversed, positive offset): a < b  <=>  key(a) < key(b)
VC_DEV uint32_t fkey(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

VC_DEV uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// uniform strictly inside (0,1) from a 32-bit hash: 23 random bits, so that (h >> 9) + 0.5 is exact in fp32 and the
// largest value is 1 - 2^-24 (with 24 bits, 16777215.5 rounds to 2^24 and u == 1 makes the Gumbel term +inf)
VC_DEV float uniform_open01(uint32_t h) { return ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f); }
// uniform in (0,1) from (seed, step, index), never 0 or 1
VC_DEV float sample_uniform(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t idx) {
    uint32_t h = mix32(idx * 0x9E3779B1u + seed_lo);
    h = mix32(h ^ (step * 0x85EBCA6Bu + seed_hi));
    return uniform_open01(h);
}

struct BlockRed {  // cross-wave scratch of the 1024-thread workgroup
    float f[16];
    int i[16];
};

VC_DEV int block_sum_i(int v, BlockRed& r, int lane, int wave) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor(v, m);
    if (lane == 0) r.i[wave] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += r.i[w];
    __syncthreads();
    return s;
}
VC_DEV float block_sum_f(float v, BlockRed& r, int lane, int wave) {
    v = wave_sum(v);
    if (lane == 0) r.f[wave] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += r.f[w];  // fixed order: bit-reproducible
    __syncthreads();
    return s;
}
VC_DEV void block_argmax(float& v, int& i, BlockRed& r, int lane, int wave) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = shfl_xor(v, m);
        const int oi = shfl_xor(i, m);
        argmax_combine2(v, i, ov, oi);
    }
    if (lane == 0) { r.f[wave] = v; r.i[wave] = i; }
    __syncthreads();
    v = r.f[0];
    i = r.i[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) argmax_combine2(v, i, r.f[w], r.i[w]);
    __syncthreads();
}

// bf16 embedding row -> fp32 residual row + sum-of-squares partials + xg = bf16(x * g) (the first GEMV's operand)
// xg_lo != nullptr (precision mode "split"): additionally the lo row bf16(x * g - xg) of the stacked hi / lo group
// sp_lo != nullptr: the lo plane of an inexact checkpoint's table row (x = hi + lo; split mode)
// chunk c (8 columns) of the row; returns the chunk's sum of squares
VC_DEV float embed_chunk_ssq(const bf16_t* sp, float* dp, const float* gw, bf16_t* xg, int c, bf16_t* xg_lo, const bf16_t* sp_lo) {
    const u32x4 v = ld16(sp + c * 8);
    f32x4 a = {bf2f_lo(v[0]), bf2f_hi(v[0]), bf2f_lo(v[1]), bf2f_hi(v[1])};
    f32x4 b = {bf2f_lo(v[2]), bf2f_hi(v[2]), bf2f_lo(v[3]), bf2f_hi(v[3])};
    if (sp_lo != nullptr) {
        const u32x4 w = ld16(sp_lo + c * 8);
        a = a + f32x4{bf2f_lo(w[0]), bf2f_hi(w[0]), bf2f_lo(w[1]), bf2f_hi(w[1])};
        b = b + f32x4{bf2f_lo(w[2]), bf2f_hi(w[2]), bf2f_lo(w[3]), bf2f_hi(w[3])};
    }
    st16f(dp + c * 8, a);
    st16f(dp + c * 8 + 4, b);
    const f32x4 g0 = ld16f(gw + c * 8), g1 = ld16f(gw + c * 8 + 4);
    const f32x4 ta = {a[0] * g0[0], a[1] * g0[1], a[2] * g0[2], a[3] * g0[3]};
    const f32x4 tb = {b[0] * g1[0], b[1] * g1[1], b[2] * g1[2], b[3] * g1[3]};
    const u32x4 hi = {pack_bf2(ta[0], ta[1]), pack_bf2(ta[2], ta[3]), pack_bf2(tb[0], tb[1]), pack_bf2(tb[2], tb[3])};
    st16(xg + c * 8, hi);
    if (xg_lo != nullptr)
        st16(xg_lo + c * 8, u32x4{pack_bf2(ta[0] - bf2f_lo(hi[0]), ta[1] - bf2f_hi(hi[0])),
                                  pack_bf2(ta[2] - bf2f_lo(hi[1]), ta[3] - bf2f_hi(hi[1])),
                                  pack_bf2(tb[0] - bf2f_lo(hi[2]), tb[1] - bf2f_hi(hi[2])),
                                  pack_bf2(tb[2] - bf2f_lo(hi[3]), tb[3] - bf2f_hi(hi[3]))});
    return ((a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3])) +
           ((b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]));
}
VC_DEV void embed_row_ssq(const bf16_t* sp, float* dp, float* ssq_row, const float* gw, bf16_t* xg, int D, int npart,
                          int lane, bf16_t* xg_lo = nullptr, const bf16_t* sp_lo = nullptr) {
    float ss = 0.f;
    for (int c = lane; c < D / 8; c += 64) ss += embed_chunk_ssq(sp, dp, gw, xg, c, xg_lo, sp_lo);
    ss = wave_sum(ss);
    for (int q = lane; q < npart; q += 64) ssq_row[q] = q == 0 ? ss : 0.f;
}

// The bookkeeping ONE selected token `sel` goes through at step `step` of its row: pad behind a finished row, EOS, the row's slot
// of the id store (`out`, RS_MAXNEW entries), the stop sequences as suffixes of (prompt tail | generated so far | the token).  -> the
// token the row emits.  The plain selection applies it to its one token, spec_accept_kernel to every token of an accepted run.
VC_DEV int emit_token(int* rs, int* out, int step, int sel) {
    const int eos = rs[RS_EOS], pad = rs[RS_PAD], nstop = rs[RS_NSTOP], max_new = rs[RS_MAXNEW];
    const bool can_finish = eos >= 0 || nstop > 0;
    const int was_finished = can_finish ? rs[RS_FINISHED] : 0;
    int tok = sel;
    if (can_finish) {
        if (was_finished) tok = pad;
        if (eos >= 0 && tok == eos) rs[RS_FINISHED] = 1;
    }
    if (step < max_new) out[step] = tok;
    if (nstop > 0 && !was_finished) {  // suffix match of the row's ids (prompt tail | generated so far | tok)
        bool hit = false;
        for (int sq = 0; sq < nstop; ++sq) {
            const int* e = rs + RS_STOP + sq * (1 + VC_MAX_STOP_LEN);
            const int L = e[0];
            bool ok = L > 0;
            for (int i = 0; i < L && ok; ++i) {
                const int back = L - 1 - i;  // 0 = the token just selected
                int v;
                if (back == 0) v = tok;
                else if (step - back >= 0) v = out[step - back];
                else v = rs[RS_TAIL + (VC_MAX_STOP_LEN - 1) + (step - back)];
                ok = v == e[1 + i];
            }
            hit = hit || ok;
        }
        if (hit) rs[RS_FINISHED] = 1;
    }
    return tok;
}

// The scaled row z = logits / temperature of a sampled selection: from its LDS staging when the row fits (lds_floats >= V), else
// recomputed from global memory in every pass — the same ROUNDED product (no contraction into the subtraction or the addition that
// consumes it: a pass that fused it would see another z than the pass that found the threshold, and the token that sits exactly on
// a typical band's tau would fall out of its own band), so both forms and all passes see the same bits.  The form is a template
// argument: every pass over the row is compiled for its form alone.
template <bool STAGED>
struct ScaledRow {
    const float* lg;
    float* zs;
    float inv_t;
    VC_DEV float operator()(int i) const {
#pragma clang fp contract(off)
        return STAGED ? zs[i] : lg[i] * inv_t;
    }
    VC_DEV void stage(int V, int tid) const {   // all threads of the workgroup
#pragma clang fp contract(off)
        if (!STAGED) return;
        for (int i = tid; i < V; i += 1024) zs[i] = lg[i] * inv_t;
        __syncthreads();
    }
};

// The kept set of a sampled row — what is left behind temperature -> top-k -> top-p -> min-p -> typical -> epsilon -> eta — as a
// predicate on the scaled VALUE: two bounds on its order-preserving key (top-k, top-p), a floor (min-p, epsilon, eta: each removes
// what lies under a probability, and the probability rises with z) and a band around the expected value (typical, below).  Equal
// values are kept or removed together, as HF's warpers do.  -inf entries (processors, an automaton) are never kept.
struct WarpSet {
    uint32_t kmin = 0;          // keep keys >= kmin (top-k)
    uint32_t kgt = 0;           // keep keys > kgt (top-p; 0 = none removed: no finite value has key 0)
    bool only_max = false;      // top_p <= 0: the draw is the argmax of what top-k left
    bool typ = false;           // the typical band applies: bits(|z - typ_c|) <= typ_tau
    float typ_c = 0.f;
    uint32_t typ_tau = 0;
    float zfloor = -INFINITY;   // keep z >= zfloor (never above the maximum of the set it was taken over)
};
VC_DEV bool warp_kept(const WarpSet& w, float v) {
    const uint32_t k = fkey(v);
    if (k < w.kmin || k <= w.kgt || !(v > -INFINITY)) return false;
    if (v < w.zfloor) return false;
    return !w.typ || __builtin_bit_cast(uint32_t, fabsf(v - w.typ_c)) <= w.typ_tau;
}

// (max, sum e, [sum e (z - max)]) over the kept set w of the row, e = exp(z - max): log Z = max + log S, H = log S - A / S
template <bool STAGED>
VC_DEV float warp_max(const ScaledRow<STAGED>& z, int V, const WarpSet& w, BlockRed& red, int tid, int lane, int wave) {
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) {
        const float v = z(i);
        if (warp_kept(w, v)) mx = fmaxf(mx, v);
    }
    int dummy = 0;
    block_argmax(mx, dummy, red, lane, wave);
    return mx;
}
template <bool STAGED>
VC_DEV void warp_mass(const ScaledRow<STAGED>& z, int V, const WarpSet& w, float mx, bool want_a, float& S, float& A, BlockRed& red, int tid,
                      int lane, int wave) {
    float s = 0.f, a = 0.f;
    for (int i = tid; i < V; i += 1024) {
        const float v = z(i);
        if (!warp_kept(w, v)) continue;
        const float e = __expf(v - mx);
        s += e;
        a += e * (v - mx);
    }
    S = block_sum_f(s, red, lane, wave);
    A = want_a ? block_sum_f(a, red, lane, wave) : 0.f;
}
// the floor that removes p < thr of a set with maximum mx and mass S (e < thr S), the maximum itself exempt
VC_DEV float warp_floor(float zfloor, float mx, float thr, float S) { return fmaxf(zfloor, fminf(mx, mx + logf(thr * S))); }

// The thresholds of the kept set of ONE sampled row under the record `rs`, in HF's warper order; every warper sees the survivors of
// those in front of it.  All 1024 threads of the workgroup call it and all get the same WarpSet; the block shape is part of the
// arithmetic (the loop strides, block_sum_f's fixed order for every mass).  A warper that is off costs its compare on the record.
//   top-k    : keep z >= the k-th largest value (bisection over the key, counting)
//   top-p    : ascending cumulative probability <= 1 - top_p is removed (bisection over the key, masses)
//   min-p    : p < min_p max p  <=>  z < max + log(min_p): no pass over the row at all
//   typical  : s_i = |-log p_i - H| = |z_i - c| with c = max + A / S, the expected value of z under p — log Z cancels.  s >= 0, so its
//              fp32 bits are an order-preserving key; tau = the largest key u with sum_{s_j < u} e_j < mass S is HF's s[last] (the
//              first entry of the ascending order whose cumulative probability reaches the mass), ties included
//   epsilon  : p < eps, eta: p < min(eta, sqrt(eta) exp(-H)) — one mass pass each (eta: with A), then a floor; the maximum of the
//              set they see is exempt, which behind a typical band need not be the row's maximum: it is taken again there
template <bool STAGED>
VC_DEV WarpSet warp_thresholds(const ScaledRow<STAGED>& z, int V, const int* rs, BlockRed& red, int tid, int lane, int wave) {
    WarpSet w;
    const int top_k = rs[RS_TOPK];
    const float top_p = __builtin_bit_cast(float, rs[RS_TOPP]);
    const float min_p = __builtin_bit_cast(float, rs[RS_MINP]), typical = __builtin_bit_cast(float, rs[RS_TYPICAL]);
    const float eps = __builtin_bit_cast(float, rs[RS_EPS]), eta = __builtin_bit_cast(float, rs[RS_ETA]);
    const bool typ_on = typical > 0.f && typical < 1.f;
    const bool more = min_p > 0.f || typ_on || eps > 0.f || eta > 0.f;
    // ---- top-k: keep z >= (k-th largest value); ties at the threshold are all kept, as TopKLogitsWarper does
    if (top_k > 0 && top_k < V) {
        uint32_t t = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            int c = 0;
            for (int i = tid; i < V; i += 1024) c += fkey(z(i)) >= cand;
            if (block_sum_i(c, red, lane, wave) >= top_k) t = cand;
        }
        w.kmin = t;
    }
    // ---- top-p over the survivors: ascending cumulative probability <= 1 - top_p is removed (TopPLogitsWarper)
    float mx = -INFINITY;   // the row's maximum: it survives top-k, top-p and min-p
    if (top_p < 1.0f || more) {
        for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, z(i));
        int dummy = 0;
        block_argmax(mx, dummy, red, lane, wave);
    }
    if (top_p < 1.0f) {
        const uint32_t kmin = w.kmin;
        float zsum = 0.f;
        for (int i = tid; i < V; i += 1024) {
            const float v = z(i);
            if (fkey(v) >= kmin) zsum += __expf(v - mx);
        }
        zsum = block_sum_f(zsum, red, lane, wave);
        const float target = (1.0f - top_p) * zsum;
        if (!(top_p > 0.f)) {
            w.only_max = true;
        } else {
            uint32_t t = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = t | (1u << bit);
                float mass = 0.f;
                for (int i = tid; i < V; i += 1024) {
                    const float v = z(i);
                    const uint32_t k = fkey(v);
                    if (k >= kmin && k <= cand) mass += __expf(v - mx);
                }
                if (block_sum_f(mass, red, lane, wave) <= target) t = cand;
            }
            w.kgt = t;
        }
    }
    if (!more || w.only_max) return w;
    // ---- min-p (MinPLogitsWarper): e < min_p, the maximum (e = 1) always kept
    if (min_p > 0.f) w.zfloor = fmaxf(w.zfloor, fminf(mx, mx + logf(min_p)));
    // ---- typical (TypicalLogitsWarper)
    if (typ_on) {
        float S, A;
        warp_mass(z, V, w, mx, true, S, A, red, tid, lane, wave);
        const float c = mx + A / S, target = typical * S;
        uint32_t t = 0;
        for (int bit = 30; bit >= 0; --bit) {   // (bit 31 is the sign: no s has it)
            const uint32_t cand = t | (1u << bit);
            float mass = 0.f;
            for (int i = tid; i < V; i += 1024) {
                const float v = z(i);
                if (warp_kept(w, v) && __builtin_bit_cast(uint32_t, fabsf(v - c)) < cand) mass += __expf(v - mx);
            }
            if (block_sum_f(mass, red, lane, wave) < target) t = cand;
        }
        w.typ = true;
        w.typ_c = c;
        w.typ_tau = t;
        if (eps > 0.f || eta > 0.f) mx = warp_max(z, V, w, red, tid, lane, wave);   // the band may have removed the maximum
    }
    // ---- epsilon (EpsilonLogitsWarper)
    if (eps > 0.f) {
        float S, A;
        warp_mass(z, V, w, mx, false, S, A, red, tid, lane, wave);
        w.zfloor = warp_floor(w.zfloor, mx, eps, S);
    }
    // ---- eta (EtaLogitsWarper): the cutoff shrinks with the entropy of what is left
    if (eta > 0.f) {
        float S, A;
        warp_mass(z, V, w, mx, true, S, A, red, tid, lane, wave);
        const float H = logf(S) - A / S;
        w.zfloor = warp_floor(w.zfloor, mx, fminf(eta, sqrtf(eta) * expf(-H)), S);
    }
    return w;
}

// the sampled selection of select_row in one staging form: the warpers, then the multinomial over the kept set as a Gumbel-max —
// argmax_i (z_i - log(-log u_i)) ~ softmax(z) restricted to it
template <bool STAGED>
VC_DEV int sample_row(const ScaledRow<STAGED>& z, int V, const int* rs, int step, BlockRed& red, int tid, int lane, int wave) {
    const uint32_t seed_lo = (uint32_t)rs[RS_SEED_LO], seed_hi = (uint32_t)rs[RS_SEED_HI];
    z.stage(V, tid);
    const WarpSet w = warp_thresholds(z, V, rs, red, tid, lane, wave);
    float best = -INFINITY;
    int bi = 0x7FFFFFFF;
    for (int i = tid; i < V; i += 1024) {
        const float v = z(i);
        if (!warp_kept(w, v)) continue;
        const float g = w.only_max ? 0.f : -__logf(-__logf(sample_uniform(seed_lo, seed_hi, (uint32_t)step, (uint32_t)i)));
        argmax_combine2(best, bi, v + g, i);
    }
    block_argmax(best, bi, red, lane, wave);
    return bi;
}

// The raw selection of ONE logits row `lg` under the record `rs` with the sampler key `step` (the generated index the token will
// have): greedy — the argmax, lowest id on ties; sampled — temperature -> the warpers of warp_thresholds -> Gumbel-max.  -> the id, in
// every thread.  Called by all 1024 threads of a workgroup; the block shape is part of the arithmetic, so select_embed_kernel and
// spec_select_kernel share this one body.  zs: the [V] LDS staging of the scaled row, used when lds_floats >= V (sampling only).
VC_DEV int select_row(const float* lg, int V, const int* rs, int step, float* zs, int lds_floats, BlockRed& red, int tid, int lane,
                      int wave) {
    float best = -INFINITY;
    int bi = 0x7FFFFFFF;
    if (!rs[RS_SAMPLE]) {
        for (int i = tid * 4; i < V; i += 4096) {
            const f32x4 v = ld16f(lg + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) argmax_combine2(best, bi, v[e], i + e);
        }
        block_argmax(best, bi, red, lane, wave);
    } else {
        const float inv_t = __builtin_bit_cast(float, rs[RS_INVTEMP]);
        bi = lds_floats >= V ? sample_row(ScaledRow<true>{lg, zs, inv_t}, V, rs, step, red, tid, lane, wave)
                             : sample_row(ScaledRow<false>{lg, zs, inv_t}, V, rs, step, red, tid, lane, wave);
    }
    return bi;
}


__global__ __launch_bounds__(1024) void select_embed_kernel(SelectArgs p) {
    VC_DYNAMIC_SMEM(float, zs);  // [V] scaled logits of the row (sampling only)
    __shared__ BlockRed red;
    __shared__ int tok_s;
    const int r = p.row0 + (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* rs = p.rows + (size_t)r * RS_STRIDE;
    if (!rs[RS_ACTIVE]) return;
    const int step = rs[RS_STEP];
    const float* lg = p.logits + (size_t)blockIdx.x * p.ldl;
    const int bi = select_row(lg, p.V, rs, step, zs, p.lds_floats, red, tid, lane, wave);
    // ---- bookkeeping (one lane) ----------------------------------------------------------------------------------
    if (tid == 0) {
        const int tok = emit_token(rs, p.out_ids + rs[RS_OUT_OFF], step, bi);
        p.next_tok[r] = tok;
        tok_s = tok;
        if (p.advance & 1) rs[RS_STEP] = step + 1;
        if (p.advance & 2) rs[RS_POS] += 1;
    }
    __syncthreads();
    if (p.embed == nullptr) return;
    const int tok = tok_s;
    const int G = p.xg_G;  // split mode: row r -> hi at row (r / G) * 2G + r % G of xg, lo G rows further
    const size_t xrow = G ? (size_t)(r / G) * 2 * G + r % G : (size_t)r;
    const bf16_t* sp = p.embed + (size_t)tok * p.D;
    const bf16_t* sp_lo = p.embed_lo ? p.embed_lo + (size_t)tok * p.D : nullptr;
    bf16_t* xg = p.xg + xrow * p.D;
    bf16_t* xg_lo = G ? p.xg + (xrow + G) * p.D : nullptr;
    const int nch = p.D / 8;
    if (nch > 1024) {   // rows wider than 8192: one wave walks the row
        if (wave == 0) embed_row_ssq(sp, p.x + (size_t)r * p.D, p.ssq + (size_t)r * p.npart, p.xg_w, xg, p.D, p.npart, lane, xg_lo, sp_lo);
        return;
    }
    // The row's 16-byte chunks over the WHOLE block, one per thread (round 6: one wave used to walk them, D / 512 dependent round
    // trips to a table row nobody has touched, on the critical path of every decode step); the sum of squares keeps its order — a
    // lane's chunks lane, lane + 64, ... added in sequence, then the wave reduction — through an LDS array of per-chunk partials
    __shared__ float part[1024];
    if (tid < nch) part[tid] = embed_chunk_ssq(sp, p.x + (size_t)r * p.D, p.xg_w, xg, tid, xg_lo, sp_lo);
    __syncthreads();
    if (wave == 0) {
        float ss = 0.f;
        for (int c = lane; c < nch; c += 64) ss += part[c];
        ss = wave_sum(ss);
        float* ssq_row = p.ssq + (size_t)r * p.npart;
        for (int q = lane; q < p.npart; q += 64) ssq_row[q] = q == 0 ? ss : 0.f;
    }
}

// ---- in-situ timing slots (vc_device.h stamp_begin / stamp_end; engine.hip vc_pool_profile) ------------------------------------
// One workgroup per launch slot: earliest start / latest end over the slot's workgroup entries (32-bit ticks: compared relative to
// one valid entry, so a wrap of the low word inside a launch does not matter), the slot re-zeroed.  The workgroup that finishes
// last (agent-scope hand-off as in decode.hip's split-K: sc1 stores, arrival counter, sc1 loads) walks the slots in launch order
// and adds, for the slot's kind — 5 slots per layer (qkv 0, attention 1, o 2, gate/up 3, down 4), the last slot lm_head (5) —
//   exec   = latest end - earliest start of the launch's workgroups, and
//   period = latest end - latest end of the PREVIOUS stamped launch of the step (the first launch: its exec): the launch as the
//            step's dependency chain pays for it, dispatch / drain / inter-kernel gap included — what bench.py's `roofline` uses
// to acc[kind] = {exec ticks, period ticks, launches}.  A slot nobody stamped (a decode attention over free rows only) is skipped.
static_assert(STAMP_SLOT_WORDS == 2 * (size_t)STAMP_WGS, "slot size");
__global__ __launch_bounds__(256) void stamp_accumulate_kernel(unsigned* stamps, int n, int layers, unsigned long long* acc,
                                                               unsigned* scratch /*[1 + 2 n]: arrival counter, {start, end} per slot*/) {
    __shared__ unsigned ref;
    __shared__ int lo, hi;
    __shared__ unsigned last;
    const int tid = threadIdx.x, j = blockIdx.x;
    unsigned* slot = stamps + (size_t)j * STAMP_SLOT_WORDS;
    if (tid == 0) {
        ref = 0;
        lo = 0x7fffffff;
        hi = -0x7fffffff;
    }
    __syncthreads();
    // all loads first (one 8-byte load per entry, issued back to back), then the re-zeroing stores: a store that depends on its own
    // load serialises the eight round trips of a thread
    u32x2 tt[STAMP_WGS / 256];
#pragma unroll
    for (int i = 0; i < STAMP_WGS / 256; ++i) tt[i] = ld8(slot + 2 * (i * 256 + tid));
    unsigned t0[STAMP_WGS / 256], t1[STAMP_WGS / 256];
#pragma unroll
    for (int i = 0; i < STAMP_WGS / 256; ++i) {
        t0[i] = tt[i][0];
        t1[i] = tt[i][1];
        if (t0[i] | t1[i]) st8(slot + 2 * (i * 256 + tid), u32x2{0u, 0u});
        if (t0[i] != 0 && t1[i] != 0) ref = t0[i];   // any valid entry serves as the reference (benign race: all are valid)
    }
    __syncthreads();
    const unsigned r = ref;
    int mylo = 0x7fffffff, myhi = -0x7fffffff;
#pragma unroll
    for (int i = 0; i < STAMP_WGS / 256; ++i)
        if (r != 0 && t0[i] != 0 && t1[i] != 0) {
            mylo = min(mylo, (int)(t0[i] - r));
            myhi = max(myhi, (int)(t1[i] - r));
        }
    if (myhi >= mylo) {
#ifdef VC_EMU
        __atomic_fetch_min(&lo, mylo, __ATOMIC_RELAXED);
        __atomic_fetch_max(&hi, myhi, __ATOMIC_RELAXED);
#else
        atomicMin(&lo, mylo);
        atomicMax(&hi, myhi);
#endif
    }
    __syncthreads();
    if (tid == 0) {
        const bool ok = r != 0 && hi >= lo;
        // {0, 0} = not stamped (a stamped end is odd: | 1 survives r + hi only by luck, so validity travels in the start word's bit 0)
        st_agent_u32(scratch + 1 + 2 * j, ok ? ((r + (unsigned)lo) | 1u) : 0u);
        st_agent_u32(scratch + 2 + 2 * j, ok ? r + (unsigned)hi : 0u);
        wait_vmcnt<0>();
        last = atomic_inc_agent(scratch) == (unsigned)(n - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    // the last arriver: all its threads fetch the per-slot results side by side (sc1 loads), one thread walks them in launch order
    constexpr int MAXS = 512;
    __shared__ unsigned sst[MAXS], sen[MAXS];
    for (int s_ = tid; s_ < n && s_ < MAXS; s_ += 256) {
        sst[s_] = ld_agent_u32(scratch + 1 + 2 * s_);
        sen[s_] = ld_agent_u32(scratch + 2 + 2 * s_);
    }
    __syncthreads();
    if (tid != 0) return;
    unsigned prev_end = 0;
    bool have_prev = false;
    unsigned long long ex[PROF_KINDS] = {}, pe[PROF_KINDS] = {}, cn[PROF_KINDS] = {};
    for (int s_ = 0; s_ < n && s_ < MAXS; ++s_) {
        const unsigned st = sst[s_], en = sen[s_];
        if (!(st & 1u)) continue;
        const int kind = s_ < 5 * layers ? s_ % 5 : 5;
        const unsigned e_ = en - (st & ~1u);
        ex[kind] += e_;
        pe[kind] += have_prev ? (unsigned)(en - prev_end) : e_;
        cn[kind] += 1;
        prev_end = en;
        have_prev = true;
    }
    for (int k = 0; k < PROF_KINDS; ++k) {   // only this thread of this launch touches acc; launches are stream-ordered
        acc[3 * k] += ex[k];
        acc[3 * k + 1] += pe[k];
        acc[3 * k + 2] += cn[k];
    }
    st_agent_u32(scratch, 0u);   // re-armed for the next step
}
void launch_stamp_accumulate(unsigned* stamps, int n, int layers, unsigned long long* acc, unsigned* scratch, hipStream_t s) {
    VC_LAUNCH(stamp_accumulate_kernel, dim3((unsigned)n), dim3(256), 0, s, stamps, n, layers, acc, scratch);
}

void launch_select_embed(const SelectArgs& a0, hipStream_t s) {
    SelectArgs a = a0;
    // the row's scaled logits are staged in LDS when they fit (sampling only reads them ~70 times)
    size_t lds = (size_t)a.V * 4;
    if (lds > 150 * 1024) lds = 0;
    a.lds_floats = (int)(lds / 4);
#ifndef VC_EMU
    static size_t allowed = 0;
    if (lds > 48 * 1024 && lds > allowed) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(select_embed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        allowed = lds;
    }
#endif
    VC_LAUNCH(select_embed_kernel, dim3(a.nrows), dim3(1024), lds, s, a);
}

// The selections of a verify step (prompt-lookup speculation under sampling or logits processors): one workgroup per verify row
// (b, j), j < nq[b], writes sel[b * Q + j] = select_row of logits row b * Q + j under record b with the sampler key RS_STEP + j — the
// key a plain step of its own would have used for the token at that generated index, so an accepted run reproduces the plain loop's
// draws id for id.  No bookkeeping: spec_accept_kernel walks `sel`.  The B * Q rows run side by side (a loop over a sequence's Q rows
// would put Q full sampler passes on the step's critical path); rows j >= nq[b] write nothing.
__global__ __launch_bounds__(1024) void spec_select_kernel(SpecSelectArgs p) {
    VC_DYNAMIC_SMEM(float, zs);  // [V] scaled logits of the row (sampling only)
    __shared__ BlockRed red;
    const int b = (int)blockIdx.x / p.Q, j = (int)blockIdx.x % p.Q, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (j >= min(p.nq[b], min(p.Q, 8))) return;
    const int* rs = p.rows + (size_t)b * RS_STRIDE;
    const int bi = select_row(p.logits + (size_t)blockIdx.x * p.ldl, p.V, rs, rs[RS_STEP] + j, zs, p.lds_floats, red, tid, lane, wave);
    if (tid == 0) p.sel[blockIdx.x] = bi;
}
void launch_spec_select(const SpecSelectArgs& a0, int lds_floats, hipStream_t s) {
    if (a0.B <= 0 || a0.Q <= 0) return;
    SpecSelectArgs a = a0;
    // staged in LDS as launch_select_embed stages its row; lds_floats < 0: what the device allows, 0 (or < V): never
    size_t lds = (size_t)a.V * 4;
    if (lds > 150 * 1024 || (lds_floats >= 0 && lds_floats < a.V)) lds = 0;
    a.lds_floats = (int)(lds / 4);
#ifndef VC_EMU
    static size_t allowed = 0;
    if (lds > 48 * 1024 && lds > allowed) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spec_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        allowed = lds;
    }
#endif
    VC_LAUNCH(spec_select_kernel, dim3((unsigned)(a.B * a.Q)), dim3(1024), lds, s, a);
}

// test hook: the sampler's hash -> uniform map on explicit hash values (the extreme h = 0xFFFFFFFF must stay below 1)
__global__ __launch_bounds__(64) void uniform_probe_kernel(const uint32_t* h, float* u, float* gumbel, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u[i] = uniform_open01(h[i]);
    gumbel[i] = -__logf(-__logf(u[i]));
}
void launch_uniform_probe(const uint32_t* h, float* u, float* gumbel, int n, hipStream_t s) {
    VC_LAUNCH(uniform_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, s, h, u, gumbel, n);
}

// test hook: the kept set of the sampled selection, from the threshold code select_row runs (same block shape, same staging)
template <bool STAGED>
VC_DEV void warp_support_row(const ScaledRow<STAGED>& z, int V, const int* rs, int* keep, BlockRed& red, int tid, int lane, int wave) {
    z.stage(V, tid);
    const WarpSet w = warp_thresholds(z, V, rs, red, tid, lane, wave);
    for (int i = tid; i < V; i += 1024) keep[i] = warp_kept(w, z(i)) ? 1 : 0;
}
__global__ __launch_bounds__(1024) void warp_support_kernel(const float* logits, int ldl, int V, const int* rows, int* keep,
                                                            int lds_floats) {
    VC_DYNAMIC_SMEM(float, zs);  // [V] scaled logits of the row
    __shared__ BlockRed red;
    const int r = (int)blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* rs = rows + (size_t)r * RS_STRIDE;
    const float* lg = logits + (size_t)r * ldl;
    const float inv_t = __builtin_bit_cast(float, rs[RS_INVTEMP]);
    if (lds_floats >= V) warp_support_row(ScaledRow<true>{lg, zs, inv_t}, V, rs, keep + (size_t)r * V, red, tid, lane, wave);
    else warp_support_row(ScaledRow<false>{lg, zs, inv_t}, V, rs, keep + (size_t)r * V, red, tid, lane, wave);
}
void launch_warp_support(const float* logits, int ldl, int V, const int* rows, int nrows, int* keep, int lds_floats, hipStream_t s) {
    if (nrows <= 0 || V <= 0) return;
    size_t lds = (size_t)V * 4;
    if (lds > 150 * 1024 || (lds_floats >= 0 && lds_floats < V)) lds = 0;
#ifndef VC_EMU
    static size_t allowed = 0;
    if (lds > 48 * 1024 && lds > allowed) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(warp_support_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        allowed = lds;
    }
#endif
    VC_LAUNCH(warp_support_kernel, dim3((unsigned)nrows), dim3(1024), lds, s, logits, ldl, V, rows, keep, (int)(lds / 4));
}

// ---- log-probability of one target token per logits row (scoring: forward(labels=), score()) -----------------------------------
//   logprob[r] = logits[r, target[r]] - logsumexp(logits[r, 0:V])       [HF] llama/modeling_llama.py: CrossEntropyLoss over the
//   shifted logits, per position and without the mean (the caller owns the reduction)
// One pass over the row: every lane keeps a running (max, sum of exp(v - max)) pair, the pairs merge through the wave (6 xor steps),
// then across the workgroup's waves through LDS, as the row kernels of norm.hip reduce.  The maximum is subtracted, so rows whose
// |logit| lies far above 88 stay finite; -inf entries (a filtered distribution) add nothing as long as one entry is finite, and a -inf
// target gives -inf.  All arithmetic fp32 (expf / logf, not the fast forms: the result is compared at the 1e-6 level).
// One workgroup per row: the callers score tens to a few thousand rows, and the 128 KB a row of V = 32000 reads takes microseconds —
// splitting a row over workgroups would buy nothing at these sizes.
// 16-byte loads where the row start allows (base and ldl multiples of 4 floats), with a scalar head up to the first aligned column
// and a scalar tail; nothing beyond column V - 1 of a row is read.
VC_DEV void lse_add(float& m, float& s, float v) {
    if (v > m) {   // (-inf never enters: m starts at -inf and v > m fails; NaN neither — a NaN logit is the caller's bug)
        s = s * expf(m - v) + 1.0f;   // m == -inf: s is 0 and expf(-inf) is 0
        m = v;
    } else if (v > -INFINITY) {
        s += expf(v - m);
    }
}
VC_DEV void lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    if (nm > -INFINITY) s = s * expf(m - nm) + os * expf(om - nm);
    m = nm;
}
constexpr int LOGPROB_THREADS = 256;
__global__ __launch_bounds__(LOGPROB_THREADS) void token_logprob_kernel(const float* __restrict__ logits, int ldl,
                                                                         const int* __restrict__ target,
                                                                         float* __restrict__ logprob, int V) {
    __shared__ float red_m[LOGPROB_THREADS / 64], red_s[LOGPROB_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lg = logits + (size_t)r * ldl;
    // columns [0, head) and [body_end, V) go one float at a time, [head, body_end) in aligned float4s
    const int mis = (int)((reinterpret_cast<uintptr_t>(lg) >> 2) & 3);
    const int head = min(V, (4 - mis) & 3);
    const int body_end = head + ((V - head) & ~3);
    float mx = -INFINITY, sm = 0.f;
    if (tid < head) lse_add(mx, sm, lg[tid]);
    for (int i = head + tid * 4; i < body_end; i += LOGPROB_THREADS * 4) {
        const f32x4 v = ld16f(lg + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) lse_add(mx, sm, v[e]);
    }
    if (body_end + tid < V) lse_add(mx, sm, lg[body_end + tid]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const float om = shfl_xor(mx, k), os = shfl_xor(sm, k);
        lse_merge(mx, sm, om, os);
    }
    if (lane == 0) { red_m[wave] = mx; red_s[wave] = sm; }
    __syncthreads();
    if (tid == 0) {
        mx = red_m[0];
        sm = red_s[0];
#pragma unroll
        for (int w = 1; w < LOGPROB_THREADS / 64; ++w) lse_merge(mx, sm, red_m[w], red_s[w]);   // fixed order: bit-reproducible
        const float t = lg[target[r]];
        logprob[r] = t > -INFINITY ? (t - mx) - logf(sm) : -INFINITY;
    }
}
void launch_token_logprob(const float* logits, int ldl, const int* target, float* logprob, int rows, int V, hipStream_t s) {
    if (rows <= 0) return;
    VC_LAUNCH(token_logprob_kernel, dim3((unsigned)rows), dim3(LOGPROB_THREADS), 0, s, logits, ldl, target, logprob, V);
}

// ---- log-probability of the chosen token and the K most likely tokens of a logits row (generate(logprobs), score(top_logprobs)) ----
//   chosen_lp[s]     = logits[r, chosen] - logsumexp(logits[r, 0:V])      (-inf logit: -inf; chosen < 0: 0.0)
//   top_ids[s, 0:K]  = the K largest logits of the row ordered by (value descending, id ascending) — ties break as the greedy
//   top_lp[s, 0:K]     argmax breaks them — each with logit - logsumexp; slots beyond the row's finite entries hold -1 / -inf
// the model's own next-token distribution (log_softmax of the fp32 logits), whatever the sampler does with it afterwards.
// One workgroup of 1024 threads per row, as select_embed_kernel, and the same exact selection: the row is staged in LDS in the pass that
// accumulates the (max, sum) pairs of token_logprob_kernel (lse_add / lse_merge, fixed merge order), the K-th largest value is found
// by bisection over the order-preserving key (32 counting passes over LDS), elements strictly above it are taken, ties at it by
// ascending id until K is reached, and one wave orders the <= 32 survivors.  No per-thread candidate lists (32 (value, id) pairs
// per thread would spill).  The survivors are gathered without atomics: every wave owns a contiguous range of ids, counts its
// entries above / at the threshold, and a second walk places them behind the counts of the waves in front of it.
// A row that does not fit the LDS staging (lds_floats < V) is re-read from global memory in every pass.
// The log-prob of an id is ONE expression, lp_value(): chosen_lp is bit-equal to the top_lp entry of the same id.
// -0.0 and +0.0 are one value to the tie rule (as to the argmax's float compare): the key maps both to +0.0's.
// rows != nullptr (the decode loop): workgroup r reads its slot from the row's record as the select kernel that just ran left it —
// step = RS_STEP - 1, token next_tok[r], slot RS_OUT_OFF + step; inactive rows and steps >= RS_MAXNEW write nothing.
VC_DEV uint32_t topk_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
constexpr uint32_t TOPK_KEY_NINF = 0x007FFFFFu;   // topk_key(-inf): every finite value lies above it
VC_DEV float lp_value(float v, float mx, float lsum) { return v > -INFINITY ? (v - mx) - lsum : -INFINITY; }
// lanes below this one whose pred holds, and (in every lane) the wave's total
VC_DEV int wave_rank(bool pred, int lane, int& total) {
#ifdef VC_EMU
    int x = pred ? 1 : 0;
    const int own = x;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = shfl(x, lane - d);
        if (lane >= d) x += o;
    }
    total = shfl(x, 63);
    return x - own;
#else
    const unsigned long long b = __builtin_amdgcn_ballot_w64(pred);
    total = __builtin_popcountll(b);
    return __builtin_popcountll(b & ((1ull << lane) - 1ull));
#endif
}
constexpr int TOPK_THREADS = 1024, TOPK_WAVES = TOPK_THREADS / 64;
__global__ __launch_bounds__(TOPK_THREADS) void topk_logprob_kernel(TopkLogprobArgs p) {
    VC_DYNAMIC_SMEM(float, zs);  // [V] the row (staged path)
    __shared__ BlockRed red;
    __shared__ float red_m[TOPK_WAVES], red_s[TOPK_WAVES];
    __shared__ int wave_gt[TOPK_WAVES], wave_eq[TOPK_WAVES];
    __shared__ float cand_v[VC_MAX_TOP_LOGPROBS];
    __shared__ int cand_i[VC_MAX_TOP_LOGPROBS];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = p.V, K = p.K;
    size_t slot = (size_t)r;
    int chosen = p.chosen ? p.chosen[r] : -1;
    if (p.rows != nullptr) {
        const int* rs = p.rows + (size_t)r * RS_STRIDE;
        if (!rs[RS_ACTIVE]) return;
        const int step = rs[RS_STEP] - 1;
        if (step < 0 || step >= rs[RS_MAXNEW]) return;
        slot = (size_t)rs[RS_OUT_OFF] + (size_t)step;
        chosen = p.next_tok[r];
    }
    const float* lg = p.logits + (size_t)r * p.ldl;
    const bool staged = K > 0 && p.lds_floats >= V;
    // ---- pass 1: (max, sum) pairs, the count of entries above -inf, the row into LDS --------------------------------------------
    // columns [0, head) and [body_end, V) go one float at a time, [head, body_end) in aligned float4s
    const int mis = (int)((reinterpret_cast<uintptr_t>(lg) >> 2) & 3);
    const int head = min(V, (4 - mis) & 3);
    const int body_end = head + ((V - head) & ~3);
    float mx = -INFINITY, sm = 0.f;
    int nfin = 0;
    auto take = [&](int i, float v) {
        lse_add(mx, sm, v);
        nfin += topk_key(v) > TOPK_KEY_NINF;
        if (staged) zs[i] = v;
    };
    if (tid < head) take(tid, lg[tid]);
    for (int i = head + tid * 4; i < body_end; i += TOPK_THREADS * 4) {
        const f32x4 v = ld16f(lg + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) take(i + e, v[e]);
    }
    if (body_end + tid < V) take(body_end + tid, lg[body_end + tid]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const float om = shfl_xor(mx, k), os = shfl_xor(sm, k);
        lse_merge(mx, sm, om, os);
    }
    if (lane == 0) { red_m[wave] = mx; red_s[wave] = sm; }
    __syncthreads();   // (also: the staged row is complete)
    mx = red_m[0];
    sm = red_s[0];
#pragma unroll
    for (int w = 1; w < TOPK_WAVES; ++w) lse_merge(mx, sm, red_m[w], red_s[w]);   // fixed order, the same in every thread
    const float lsum = logf(sm);
    if (tid == 0 && p.chosen_lp != nullptr)
        p.chosen_lp[slot] = (unsigned)chosen < (unsigned)V ? lp_value(lg[chosen], mx, lsum) : 0.0f;
    if (K <= 0) return;
    float* out_lp = p.top_lp + slot * (size_t)K;
    int* out_id = p.top_ids + slot * (size_t)K;
    const int keff = min(K, block_sum_i(nfin, red, lane, wave));
    if (keff == 0) {
        if (tid < K) { out_lp[tid] = -INFINITY; out_id[tid] = -1; }
        return;
    }
    auto z = [&](int i) { return staged ? zs[i] : lg[i]; };
    // ---- the keff-th largest key: the largest t with count(key >= t) >= keff (above TOPK_KEY_NINF, as keff entries are) ---------
    uint32_t t = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        int c = 0;
        for (int i = tid; i < V; i += TOPK_THREADS) c += topk_key(z(i)) >= cand;
        if (block_sum_i(c, red, lane, wave) >= keff) t = cand;
    }
    // ---- gather: wave w owns ids [w * seg, (w + 1) * seg) ------------------------------------------------------------------------
    const int seg = (((V + TOPK_WAVES - 1) / TOPK_WAVES) + 63) & ~63;
    const int i0 = wave * seg, i1 = min(V, i0 + seg);
    int cg = 0, ce = 0;
    for (int i = i0 + lane; i < i1; i += 64) {
        const uint32_t k = topk_key(z(i));
        cg += k > t;
        ce += k == t;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        cg += shfl_xor(cg, m);
        ce += shfl_xor(ce, m);
    }
    if (lane == 0) { wave_gt[wave] = cg; wave_eq[wave] = ce; }
    __syncthreads();
    int goff = 0, eoff = 0, total_gt = 0;
    for (int w = 0; w < TOPK_WAVES; ++w) {
        if (w < wave) { goff += wave_gt[w]; eoff += wave_eq[w]; }
        total_gt += wave_gt[w];
    }
    const int need = keff - total_gt;   // ties taken at the threshold, by ascending id (>= 1: count(key > t) < keff)
    for (int b = i0; b < i1; b += 64) {   // (wave-uniform trip count: every lane takes part in the ranks)
        const int i = b + lane;
        const bool in = i < i1;
        const float v = in ? z(i) : 0.f;
        const uint32_t k = in ? topk_key(v) : 0u;
        int ng, ne;
        const int rg = goff + wave_rank(in && k > t, lane, ng);
        const int re = eoff + wave_rank(in && k == t, lane, ne);
        int s_ = -1;
        if (in && k > t) s_ = rg;
        else if (in && k == t && re < need) s_ = total_gt + re;
        if (s_ >= 0 && s_ < VC_MAX_TOP_LOGPROBS) { cand_v[s_] = v; cand_i[s_] = i; }
        goff += ng;
        eoff += ne;
    }
    __syncthreads();
    // ---- one wave orders the keff survivors: rank = survivors in front by (value descending, id ascending) -----------------------
    if (wave != 0 || lane >= K) return;
    if (lane >= keff) {
        out_lp[lane] = -INFINITY;
        out_id[lane] = -1;
        return;
    }
    const float v = cand_v[lane];
    const int id = cand_i[lane];
    int rank = 0;
    for (int o = 0; o < keff; ++o) {
        const float ov = cand_v[o];
        const int oi = cand_i[o];
        rank += ov > v || (ov == v && oi < id);
    }
    out_lp[rank] = lp_value(v, mx, lsum);
    out_id[rank] = id;
}
void launch_topk_logprob(const TopkLogprobArgs& a0, int nrows, int lds_floats, hipStream_t s) {
    if (nrows <= 0) return;
    TopkLogprobArgs a = a0;
    // the row is staged in LDS when it fits (the selection reads it ~35 times); lds_floats < 0: what the device allows
    size_t lds = (size_t)a.V * 4;
    if (lds > 150 * 1024 || a.K <= 0 || (lds_floats >= 0 && lds_floats < a.V)) lds = 0;
    a.lds_floats = (int)(lds / 4);
#ifndef VC_EMU
    static size_t allowed = 0;
    if (lds > 48 * 1024 && lds > allowed) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_logprob_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        allowed = lds;
    }
#endif
    VC_LAUNCH(topk_logprob_kernel, dim3((unsigned)nrows), dim3(TOPK_THREADS), lds, s, a);
}

// ---- logits processors in front of the selection (generate(repetition_penalty=, no_repeat_ngram_size=, bad_words_ids=,
// min_new_tokens= / min_length=); [HF] generation/logits_process.py of Transformers 4.31) ------------------------------------------
// One workgroup of 1024 threads per row writes a processed copy of the raw fp32 row; the raw row is only read (the log-prob kernel
// keeps scoring it).  Every processor touches a sparse set of entries chosen by the row's own history h = the caller's prompt ids
// (placeholders and all: HF counts the un-spliced input_ids) followed by out_ids[0 .. RS_STEP), of length L.  Four phases, a
// workgroup barrier between them:
//   1. copy: 16-byte accesses over the part of the row where source and destination are both aligned, scalar elsewhere
//   2. RepetitionPenaltyLogitsProcessor: out[t] = raw[t] < 0 ? raw[t] * p : raw[t] / p for every history id t in [0, V) — read from
//      the RAW row, so the duplicates of a history write the same bits, and an IEEE division (no reciprocal): numpy float32
//      reproduces it.  HF would raise an index error on the image placeholders (negative ids); they are skipped here.
//   3. -inf setters, in any order (a token both penalised and banned ends as -inf: the barrier stands between the two writes):
//      NoRepeatNGramLogitsProcessor (size n; L + 1 >= n): h[i + n - 1] for every start 0 <= i <= L - n whose n - 1 ids equal the
//        last n - 1 of the history; the starts are spread over the threads; n = 1 bans every history id
//      NoBadWordsLogitsProcessor: sequence q of the call's table (thread q): one id — always; longer — its last id when the
//        history ends with the ids in front of it (a tail that may reach into the prompt)
//      MinNewTokensLengthLogitsProcessor / MinLengthLogitsProcessor (folded on the host): RS_EOS and RS_LP_EOS while RS_STEP < m
//   4. the token automaton (LogitsProcessArgs::cn_*; records with RS_CN_ON, unfinished, plain form): thread 0 advances the row's
//      state over out_ids[RS_CN_POS .. RS_STEP) — a binary search in the state's edge slice per id, else default_next — stores
//      (state, RS_STEP) back and broadcasts it through LDS.  A free-text state (default_next >= 0) masks nothing; the dead state
//      fills [0, V) with -inf; otherwise the workgroup sets one bit per allowed id in an LDS bitmap (the state's edge slice read once,
//      a run of consecutive edges per thread; two barriers), and every thread takes 4-float chunks of `out` (16-byte accesses over the aligned part): a chunk
//      whose ids are all allowed is not touched, one with none is stored as -inf without a load, the rest is read, masked, stored.
//      No cap on a state's edges; a thread touches its own chunks only, behind the barrier that ends phase 3.  A vocabulary above
//      32 * CN_BITMAP_WORDS ids takes lower_bound(chunk start) in the sorted slice per chunk instead of the bitmap.
// Ids outside [0, V) are never written.  Rows are independent; pad columns V .. ldo are not touched.
// The verify form (p.Q > 0; prompt-lookup speculation): workgroup r = b * Q + j, j < nq[b], processes logits row r under record b as
// the plain loop would j steps later, if the j drafts in front of the row are accepted — the history is followed by the drafts
// tok[b * Q + 1 .. b * Q + j] (tok[b * Q] is out_ids[RS_STEP - 1], in the store already) and MinNewTokens compares RS_STEP + j.  Rows
// j >= nq[b] write nothing.  A row behind a rejected draft holds what nobody reads.
constexpr int LPROC_THREADS = 1024;
constexpr int CN_BITMAP_WORDS = 8192;   // 32 KB of LDS: one bit per id of a vocabulary of up to 262144
// the token automaton of phase 4: first edge of [e0, e1) whose id is >= t; the state behind `tok` in state `st`
VC_DEV int cn_lower_bound(const int* et, int e0, int e1, int t) {
    while (e0 < e1) {
        const int mid = e0 + ((e1 - e0) >> 1);
        if (et[mid] < t) e0 = mid + 1;
        else e1 = mid;
    }
    return e0;
}
VC_DEV int cn_step(const LogitsProcessArgs& p, int st, int tok) {
    if ((unsigned)st >= (unsigned)p.cn_states) return -1;
    const int e1 = p.cn_state_off[st + 1], k = cn_lower_bound(p.cn_edge_tok, p.cn_state_off[st], e1, tok);
    return k < e1 && p.cn_edge_tok[k] == tok ? p.cn_edge_next[k] : p.cn_default_next[st];
}
__global__ __launch_bounds__(LPROC_THREADS) void logits_process_kernel(LogitsProcessArgs p) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int rec = p.Q > 0 ? r / p.Q : r, nd = p.Q > 0 ? r % p.Q : 0;   // the row's record; the drafts behind its history
    if (p.Q > 0 && nd >= min(p.nq[rec], p.Q)) return;
    const int* rs = p.rows + (size_t)rec * RS_STRIDE;
    if (!rs[RS_ACTIVE]) return;
    const int V = p.V;
    const float* lg = p.logits + (size_t)r * p.ldl;
    float* out = p.out + (size_t)r * p.ldo;
    // ---- 1. copy ----------------------------------------------------------------------------------------------------------------
    const int mis = (int)((reinterpret_cast<uintptr_t>(lg) >> 2) & 3);
    const bool vec = ((reinterpret_cast<uintptr_t>(lg) ^ reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int head = vec ? min(V, (4 - mis) & 3) : V;   // columns [0, head) and [body_end, V) one float at a time
    const int body_end = head + ((V - head) & ~3);
    for (int i = tid; i < head; i += LPROC_THREADS) out[i] = lg[i];
    for (int i = head + tid * 4; i < body_end; i += LPROC_THREADS * 4) st16f(out + i, ld16f(lg + i));
    if (body_end + tid < V) out[body_end + tid] = lg[body_end + tid];
    // ---- the row's history ------------------------------------------------------------------------------------------------------
    const int P = max(rs[RS_LP_HIST_LEN], 0);
    const int step = max(min(rs[RS_STEP], rs[RS_MAXNEW]), 0);
    const int G = P + step, L = G + nd;
    const int* hp = p.prompt_ids + rs[RS_LP_HIST_OFF];
    const int* hg = p.out_ids + rs[RS_OUT_OFF];
    const int* hd = nd > 0 ? p.tok + (size_t)rec * p.Q + 1 : nullptr;
    auto h = [&](int j) { return j < P ? hp[j] : (j < G ? hg[j - P] : hd[j - G]); };
    const float pen = __builtin_bit_cast(float, rs[RS_LP_PENALTY]);
    const int n = rs[RS_LP_NGRAM], nbad = p.bad_words != nullptr ? min(rs[RS_LP_NBAD], VC_MAX_BAD_WORDS) : 0;
    __syncthreads();
    // ---- 2. repetition penalty --------------------------------------------------------------------------------------------------
    if (pen > 0.f && pen != 1.0f) {
        for (int j = tid; j < L; j += LPROC_THREADS) {
            const int t = h(j);
            if ((unsigned)t >= (unsigned)V) continue;
            const float v = lg[t];
            out[t] = v < 0.f ? v * pen : v / pen;
        }
    }
    __syncthreads();
    // ---- 3. -inf setters --------------------------------------------------------------------------------------------------------
    if (n >= 1 && L + 1 >= n) {
        const int tail0 = L - n + 1;   // the last n - 1 ids: h[tail0 .. L)
        for (int i = tid; i <= L - n; i += LPROC_THREADS) {
            bool ok = true;
            for (int k = 0; k < n - 1 && ok; ++k) ok = h(i + k) == h(tail0 + k);
            const int t = h(i + n - 1);
            if (ok && (unsigned)t < (unsigned)V) out[t] = -INFINITY;
        }
    }
    if (tid < nbad) {
        const int* e = p.bad_words + tid * (1 + VC_MAX_BAD_WORD_LEN);
        const int len = e[0];
        bool ok = len >= 1 && len <= VC_MAX_BAD_WORD_LEN && len - 1 <= L;
        for (int k = 0; k < len - 1 && ok; ++k) ok = h(L - (len - 1) + k) == e[1 + k];
        if (ok && (unsigned)e[len] < (unsigned)V) out[e[len]] = -INFINITY;
    }
    if (rs[RS_STEP] + nd < rs[RS_LP_MINNEW]) {
        const int neos = min(rs[RS_LP_NEOS], VC_MAX_EOS_EXTRA);
        if (tid <= neos) {
            const int t = tid == 0 ? rs[RS_EOS] : rs[RS_LP_EOS + tid - 1];
            if ((unsigned)t < (unsigned)V) out[t] = -INFINITY;
        }
    }
    // ---- 4. the token automaton (PrefixConstrainedLogitsProcessor: behind MinNewTokensLength) --------------------------------------
    if (p.cn_state_off == nullptr || p.Q > 0 || !rs[RS_CN_ON] || rs[RS_FINISHED]) return;   // (uniform over the workgroup)
    __shared__ int cn_state_s;
    if (tid == 0) {
        // the stored state is a cache of walk(out_ids[0 .. RS_STEP)): advance it over the ids emitted since (one, as a rule)
        int* rw = p.rows + (size_t)rec * RS_STRIDE;
        int st = rs[RS_CN_STATE], pos = rs[RS_CN_POS];
        if (pos < 0 || pos > step) st = 0, pos = 0;
        for (; pos < step; ++pos) st = cn_step(p, st, hg[pos]);
        if ((unsigned)st >= (unsigned)p.cn_states) st = -1;   // one dead state
        rw[RS_CN_STATE] = st;
        rw[RS_CN_POS] = step;
        cn_state_s = st;
    }
    __syncthreads();   // the state; and phase 3's writes are behind it
    const int st = cn_state_s;
    const bool dead = (unsigned)st >= (unsigned)p.cn_states;
    if (!dead && p.cn_default_next[st] >= 0) return;   // free text: the edges only redirect
    const int e0 = dead ? 0 : p.cn_state_off[st], e1 = dead ? 0 : p.cn_state_off[st + 1];
    const int* et = p.cn_edge_tok;
    // in place on `out`: a thread owns the ids of its chunks, scalar in front of and behind the 16-byte aligned part of the row
    const int omis = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
    const int ohead = min(V, (4 - omis) & 3), obody_end = ohead + ((V - ohead) & ~3);
    const f32x4 ninf4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (((V + 31) >> 5) <= CN_BITMAP_WORDS) {
        // the state's allowed ids as a bitmap in LDS: the edges are read once, with no search (a binary search per chunk is
        // a chain of dependent loads: a launch of 20.6 us for 133 edges, against 8.6 us this way)
        __shared__ unsigned allowed[CN_BITMAP_WORDS];
        for (int w = tid; w < ((V + 31) >> 5); w += LPROC_THREADS) allowed[w] = 0u;
        __syncthreads();
        // a thread takes a run of consecutive edges and gathers the bits of one word before it touches LDS: the ids of a dense state
        // fall into the same few words, and one atomic per edge would serialise a wave on them (33 us for 32000 edges, 20 us this way)
        auto flush = [&](int w, unsigned bits) {
            if (bits == 0u) return;
#ifdef VC_EMU
            __atomic_fetch_or(&allowed[w], bits, __ATOMIC_RELAXED);
#else
            atomicOr(&allowed[w], bits);
#endif
        };
        const int per = (e1 - e0 + LPROC_THREADS - 1) / LPROC_THREADS;
        const int eb = e0 + tid * per, ee = min(eb + per, e1);
        int w = 0;
        unsigned bits = 0u;
        for (int e = eb; e < ee; ++e) {
            const int t = et[e];
            if ((unsigned)t >= (unsigned)V) continue;
            if ((t >> 5) != w) {
                flush(w, bits);
                w = t >> 5;
                bits = 0u;
            }
            bits |= 1u << (t & 31);
        }
        flush(w, bits);
        __syncthreads();
        auto ok = [&](int i) { return (allowed[i >> 5] >> (i & 31)) & 1u; };
        if (tid < ohead && !ok(tid)) out[tid] = -INFINITY;
        for (int i = ohead + tid * 4; i < obody_end; i += LPROC_THREADS * 4) {
            const unsigned m = ok(i) | ok(i + 1) << 1 | ok(i + 2) << 2 | ok(i + 3) << 3;
            if (m == 15u) continue;          // every id of the chunk is allowed: not touched
            if (m == 0u) {                   // none: written without being read
                st16f(out + i, ninf4);
                continue;
            }
            f32x4 v = ld16f(out + i);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (!(m >> c & 1u)) v[c] = -INFINITY;
            st16f(out + i, v);
        }
        if (obody_end + tid < V && !ok(obody_end + tid)) out[obody_end + tid] = -INFINITY;
        return;
    }
    // a vocabulary the bitmap does not hold: every thread finds lower_bound(chunk start) in the sorted slice
    auto one = [&](int i) {
        const int k = cn_lower_bound(et, e0, e1, i);
        if (k >= e1 || et[k] != i) out[i] = -INFINITY;
    };
    if (tid < ohead) one(tid);
    for (int i = ohead + tid * 4; i < obody_end; i += LPROC_THREADS * 4) {
        int k = cn_lower_bound(et, e0, e1, i);
        if (k >= e1 || et[k] >= i + 4) {
            st16f(out + i, ninf4);
            continue;
        }
        f32x4 v = ld16f(out + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (k < e1 && et[k] == i + c) ++k;
            else v[c] = -INFINITY;
        }
        st16f(out + i, v);
    }
    if (obody_end + tid < V) one(obody_end + tid);
}
void launch_logits_process(const LogitsProcessArgs& a, int nrows, hipStream_t s) {
    if (nrows <= 0) return;
    VC_LAUNCH(logits_process_kernel, dim3((unsigned)nrows), dim3(LPROC_THREADS), 0, s, a);
}

// ---- classifier-free guidance in front of the processors (generate(guidance_scale=, negative_prompt_ids=); [HF]
// generation/logits_process.py UnbatchedClassifierFreeGuidanceLogitsProcessor) --------------------------------------------------------
// One workgroup of 1024 threads per pair (conditional row c, unconditional row u), two passes:
//   1. the (max, sum) pairs of BOTH rows with lse_add / lse_merge in the fixed merge order of token_logprob_kernel (lanes, then the
//      waves in ascending order, the same in every thread), one partition of the columns for both rows — identical rows reduce to
//      identical scalars;
//   2. out[t] = g * (lc[t] - lu[t]) + lu[t] with lc[t] = (c[t] - max c) - log sum c, lu likewise — lp_value()'s expression — the
//      product and the sum rounded separately (guided_value: contraction off), so numpy float32 reproduces every bit from the four
//      scalars, which tid 0 leaves in scalars[r].
// Two rows of V = 32000 (250 KiB) do not fit a CU's LDS together, and NEITHER is staged: both were just written by the lm_head launch
// and sit in L2, so pass 2 re-reads them from there — staging the conditional row in 16-byte LDS accesses measured 25.6 us per launch
// against 25.6 us without at V = 32000, B = 1 (profiles/guidance_wall_times.md), and without it the kernel needs no dynamic LDS.
// 16-byte accesses over [head, body_end) where the rows are congruent modulo 16 bytes (pass 1: c and u; pass 2: `out` too), one float
// at a time in front of and behind it, and everywhere when they are not; nothing beyond column V - 1 is read, pad columns of `out`
// are not written.
constexpr int GUIDE_THREADS = 1024, GUIDE_WAVES = GUIDE_THREADS / 64;
VC_DEV float guided_value(float c, float u, float mc, float lsc, float mu, float lsu, float g) {
#pragma clang fp contract(off)
    const float lc = (c - mc) - lsc;
    const float lu = (u - mu) - lsu;
    const float d = lc - lu;
    const float p = g * d;
    return p + lu;
}
__global__ __launch_bounds__(GUIDE_THREADS) void guidance_combine_kernel(GuidanceCombineArgs p) {
    __shared__ float red_mc[GUIDE_WAVES], red_sc[GUIDE_WAVES], red_mu[GUIDE_WAVES], red_su[GUIDE_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* rs = p.rows + (size_t)r * RS_STRIDE;
    if (!rs[RS_ACTIVE]) return;
    const int V = p.V;
    const float g = __builtin_bit_cast(float, rs[RS_GD_SCALE]);
    const float* c = p.cond + (size_t)r * p.ldl;
    const float* u = p.uncond + (size_t)r * p.ldl;
    float* out = p.out + (size_t)r * p.ldo;
    // ---- pass 1 -------------------------------------------------------------------------------------------------------------------
    const int mis = (int)((reinterpret_cast<uintptr_t>(c) >> 2) & 3);
    const bool vec1 = ((reinterpret_cast<uintptr_t>(c) ^ reinterpret_cast<uintptr_t>(u)) & 15) == 0;
    const bool vec2 = vec1 && ((reinterpret_cast<uintptr_t>(c) ^ reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int head = vec1 ? min(V, (4 - mis) & 3) : V;   // columns [0, head) and [body_end, V) one float at a time
    const int body_end = head + ((V - head) & ~3);
    float mc = -INFINITY, sc = 0.f, mu = -INFINITY, su = 0.f;
    for (int i = tid; i < head; i += GUIDE_THREADS) {
        lse_add(mc, sc, c[i]);
        lse_add(mu, su, u[i]);
    }
    for (int i = head + tid * 4; i < body_end; i += GUIDE_THREADS * 4) {
        const f32x4 cv = ld16f(c + i), uv = ld16f(u + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lse_add(mc, sc, cv[e]);
            lse_add(mu, su, uv[e]);
        }
    }
    if (body_end + tid < V) {
        lse_add(mc, sc, c[body_end + tid]);
        lse_add(mu, su, u[body_end + tid]);
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const float omc = shfl_xor(mc, k), osc = shfl_xor(sc, k), omu = shfl_xor(mu, k), osu = shfl_xor(su, k);
        lse_merge(mc, sc, omc, osc);
        lse_merge(mu, su, omu, osu);
    }
    if (lane == 0) { red_mc[wave] = mc; red_sc[wave] = sc; red_mu[wave] = mu; red_su[wave] = su; }
    __syncthreads();
    mc = red_mc[0];
    sc = red_sc[0];
    mu = red_mu[0];
    su = red_su[0];
#pragma unroll
    for (int w = 1; w < GUIDE_WAVES; ++w) {   // fixed order, the same in every thread
        lse_merge(mc, sc, red_mc[w], red_sc[w]);
        lse_merge(mu, su, red_mu[w], red_su[w]);
    }
    const float lsc = logf(sc), lsu = logf(su);
    if (tid == 0) {
        float* q = p.scalars + (size_t)r * 4;
        q[0] = mc;
        q[1] = lsc;
        q[2] = mu;
        q[3] = lsu;
    }
    // ---- pass 2 -------------------------------------------------------------------------------------------------------------------
    const int head2 = vec2 ? head : V, body_end2 = vec2 ? body_end : V;
    for (int i = tid; i < head2; i += GUIDE_THREADS) out[i] = guided_value(c[i], u[i], mc, lsc, mu, lsu, g);
    for (int i = head2 + tid * 4; i < body_end2; i += GUIDE_THREADS * 4) {
        const f32x4 cv = ld16f(c + i), uv = ld16f(u + i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = guided_value(cv[e], uv[e], mc, lsc, mu, lsu, g);
        st16f(out + i, o);
    }
    if (body_end2 + tid < V) out[body_end2 + tid] = guided_value(c[body_end2 + tid], u[body_end2 + tid], mc, lsc, mu, lsu, g);
}
void launch_guidance_combine(const GuidanceCombineArgs& a, int nrows, hipStream_t s) {
    if (nrows <= 0) return;
    VC_LAUNCH(guidance_combine_kernel, dim3((unsigned)nrows), dim3(GUIDE_THREADS), 0, s, a);
}

// The unconditional rows of a guided step follow their partners: behind select_embed_kernel over rows 0 .. B - 1, workgroup i copies
// what that launch left for row i — next_tok, the fp32 residual row, its sum-of-squares partials, the first GEMV's operand row — to
// row B + i, mirrors RS_FINISHED and advances row B + i's OWN RS_STEP / RS_POS (the two prompts differ in length).  A follower
// records no ids (its RS_MAXNEW is 0) and is never selected for.  16-byte copies: D is a multiple of 8, the rows start on 16 bytes.
__global__ __launch_bounds__(256) void guidance_follow_kernel(GuidanceFollowArgs p) {
    const int src = blockIdx.x, dst = p.B + (int)blockIdx.x, tid = threadIdx.x;
    int* rs = p.rows + (size_t)dst * RS_STRIDE;
    if (!rs[RS_ACTIVE]) return;
    const float* xs = p.x + (size_t)src * p.D;
    float* xd = p.x + (size_t)dst * p.D;
    for (int i = tid * 4; i < p.D; i += 256 * 4) st16f(xd + i, ld16f(xs + i));
    const bf16_t* gs = p.xg + (size_t)src * p.D;
    bf16_t* gd = p.xg + (size_t)dst * p.D;
    for (int i = tid * 8; i < p.D; i += 256 * 8) st16(gd + i, ld16(gs + i));
    for (int q = tid; q < p.npart; q += 256) p.ssq[(size_t)dst * p.npart + q] = p.ssq[(size_t)src * p.npart + q];
    if (tid == 0) {
        p.next_tok[dst] = p.next_tok[src];
        rs[RS_FINISHED] = p.rows[(size_t)src * RS_STRIDE + RS_FINISHED];
        if (p.advance & 1) rs[RS_STEP] += 1;
        if (p.advance & 2) rs[RS_POS] += 1;
    }
}
void launch_guidance_follow(const GuidanceFollowArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    VC_LAUNCH(guidance_follow_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
}

// ---- one beam-search step on the device (kernels.h BeamStepArgs; [HF] generation/utils.py beam_search + beam_search.py
// BeamSearchScorer.process of Transformers 4.31) -----------------------------------------------------------------------------------
// ONE workgroup, one wave per sequence (B * n <= 16 rows, so the launch holds at most 16 * 32 = 512 candidates): the lanes add
// the running beam score to the candidates and rank them by counting (score descending, then (row, id) ascending — the flat index
// beam * V + id, the argmax's tie rule; a score the -1e9 of an unborn beam swallowed ties with its neighbours), lane 0 then walks
// the 2 n best in rank order exactly as the host loop does.  All arithmetic is one fp32 add and fp32 divisions by tabulated
// denominators: a numpy float32 restatement reproduces every bit.  Clarity over occupancy: a few hundred candidates per step.
VC_DEV bool beam_before(float s, int row, int id, float os, int orow, int oid) {   // (os, orow, oid) ranks in front of (s, row, id)
    return os > s || (os == s && (orow < row || (orow == row && oid < id)));
}
__global__ __launch_bounds__(1024) void beam_step_kernel(BeamStepArgs p) {
    constexpr int MAXC = VC_BEAM_MAX_ROWS * VC_MAX_TOP_LOGPROBS;
    __shared__ float c_s[MAXC];
    __shared__ int c_i[MAXC];
    __shared__ int top_c[2 * VC_BEAM_MAX_ROWS];   // per sequence: candidate index by rank, -1 behind the last candidate
    const int tid = threadIdx.x, lane = tid & 63, b = tid >> 6;
    const int n = p.n, K = 2 * n, nc = n * K, R = p.B * n, base = b * nc;
    for (int c = lane; c < nc; c += 64) {
        const int id = p.cand_id[base + c];
        c_i[base + c] = id;
        c_s[base + c] = id >= 0 ? p.cand_lp[base + c] + p.beam_score[b * n + c / K] : -INFINITY;
    }
    if (lane < K) top_c[b * K + lane] = -1;
    __syncthreads();
    for (int c = lane; c < nc; c += 64) {
        const int id = c_i[base + c];
        if (id < 0) continue;
        const float s = c_s[base + c];
        int rank = 0;
        for (int o = 0; o < nc; ++o) {
            const int oid = c_i[base + o];
            rank += oid >= 0 && beam_before(s, c / K, id, c_s[base + o], o / K, oid);
        }
        if (rank < K) top_c[b * K + rank] = c;
    }
    __syncthreads();
    if (lane == 0) {
        int* sq = p.seq + b * BQ_STRIDE;
        int* hyp = p.hyp + (size_t)b * n * BH_STRIDE;
        const int step = p.rows[(size_t)b * n * RS_STRIDE + RS_STEP];
        const bool live = step >= 0 && step < p.params[BP_MAXNEW] && !sq[BQ_DONE];
        const int pad = p.params[BP_PAD];
        int k = 0;
        auto emit = [&](float score, int tok, int src) {   // beam slot k of the sequence
            const int r = b * n + k;
            p.beam_score[r] = score;
            p.next_tok[r] = tok;
            p.perm[r] = src;
            if (step >= 0 && step < p.params[BP_MAXNEW]) {
                p.tok_tab[(size_t)step * R + r] = tok;
                p.parent_tab[(size_t)step * R + r] = src;
            }
            ++k;
        };
        if (live) {
            const int n_eos = p.params[BP_N_EOS];
            for (int rank = 0; rank < K && k < n; ++rank) {
                const int c = top_c[b * K + rank];
                if (c < 0) break;
                const int id = c_i[base + c], src = b * n + c / K;
                const float sum = c_s[base + c];
                bool is_eos = false;
                for (int e = 0; e < n_eos; ++e) is_eos = is_eos || id == p.params[BP_EOS + e];
                if (!is_eos) {
                    emit(sum, id, src);
                    continue;
                }
                if (rank >= n) continue;
                // BeamHypotheses.add: kept while fewer than n are held or it beats the worst; the worst (the first of equals) leaves
                const float score = sum / p.hyp_den[step];
                int nh = sq[BQ_NHYP];
                float worst = __builtin_bit_cast(float, sq[BQ_WORST]);
                if (nh >= n && !(score > worst)) continue;
                if (nh >= n) {
                    int lo = 0;
                    for (int j = 1; j < nh; ++j)
                        if (__builtin_bit_cast(float, hyp[j * BH_STRIDE + BH_SCORE]) < __builtin_bit_cast(float, hyp[lo * BH_STRIDE + BH_SCORE])) lo = j;
                    for (int j = lo; j + 1 < nh; ++j)
                        for (int q = 0; q < BH_STRIDE; ++q) hyp[j * BH_STRIDE + q] = hyp[(j + 1) * BH_STRIDE + q];
                    --nh;
                }
                hyp[nh * BH_STRIDE + BH_SCORE] = __builtin_bit_cast(int, score);
                hyp[nh * BH_STRIDE + BH_SUM] = __builtin_bit_cast(int, sum);
                hyp[nh * BH_STRIDE + BH_STEP] = step;
                hyp[nh * BH_STRIDE + BH_ROW] = src;
                ++nh;
                worst = score;
                for (int j = 0; j < nh; ++j) worst = fminf(worst, __builtin_bit_cast(float, hyp[j * BH_STRIDE + BH_SCORE]));
                sq[BQ_NHYP] = nh;
                sq[BQ_WORST] = __builtin_bit_cast(int, worst);
            }
            if (k < n) p.flags[1] = 1;   // more than n EOS among the 2 n best (or too few candidates): the host raises
            // BeamHypotheses.is_done against the best candidate of the step
            const int c0 = top_c[b * K];
            const float best = c0 >= 0 ? c_s[base + c0] : -INFINITY;
            const int early = p.params[BP_EARLY];
            if (sq[BQ_NHYP] >= n && (early == 1 || __builtin_bit_cast(float, sq[BQ_WORST]) >= best / p.done_den[step])) {
                sq[BQ_DONE] = 1;
                sq[BQ_DONE_STEP] = step;
            }
        }
        while (k < n) emit(0.f, pad, b * n + k);   // a done sequence (and the slots an error left open): pad, its own row
        for (int j = 0; j < n; ++j) {
            int* rs = p.rows + (size_t)(b * n + j) * RS_STRIDE;
            if (p.advance & 1) rs[RS_STEP] = step + 1;
            if (p.advance & 2) rs[RS_POS] += 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int all = 1;
        for (int q = 0; q < p.B; ++q) all = all && p.seq[q * BQ_STRIDE + BQ_DONE];
        p.flags[0] = all;
    }
}
void launch_beam_step(const BeamStepArgs& a, hipStream_t s) {
    if (a.B < 1 || a.n < 1 || a.B * a.n > VC_BEAM_MAX_ROWS) return;   // nothing is launched, nothing written
    VC_LAUNCH(beam_step_kernel, dim3(1), dim3(64 * a.B), 0, s, a);
}

// embedding + sum-of-squares partials for tokens supplied by the host (vc_decode_step with explicit tokens)
__global__ __launch_bounds__(256) void embed_tokens_ssq_kernel(const int* tok, const bf16_t* embed, float* x, float* ssq,
                                                               const float* xg_w, bf16_t* xg, int B, int D, int npart, int G,
                                                               const bf16_t* embed_lo) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const size_t xrow = G ? (size_t)(row / G) * 2 * G + row % G : (size_t)row;
    embed_row_ssq(embed + (size_t)tok[row] * D, x + (size_t)row * D, ssq + (size_t)row * npart, xg_w, xg + xrow * D, D,
                  npart, threadIdx.x & 63, G ? xg + (xrow + G) * D : nullptr, embed_lo ? embed_lo + (size_t)tok[row] * D : nullptr);
}
void launch_embed_tokens_ssq(const int* tok, const bf16_t* embed, float* x, float* ssq, const float* xg_w, bf16_t* xg, int B,
                             int D, int npart, hipStream_t s, int xg_G, const bf16_t* embed_lo) {
    VC_LAUNCH(embed_tokens_ssq_kernel, dim3((B + 3) / 4), dim3(256), 0, s, tok, embed, x, ssq, xg_w, xg, B, D, npart, xg_G, embed_lo);
}

// ---- prompt-lookup speculation: the draft in front of a verify step, the acceptance behind its lm_head ---------------------------
// The corpus of sequence b: its lookup ids | a separator no window may touch | its prompt ids | the ids it has generated.  For
// ng = max_ngram .. 1 (an ng longer than prompt + generated is not tried) the last ng ids are sought at every earlier start; the
// latest match of the first ng that has one decides, and the ids behind it are the drafts: at most k, cut at the corpus end and at the
// first id that is no vocabulary id (the separator, a placeholder of the prompt).  One workgroup per sequence: every thread tries the
// starts tid, tid + 256, ..., the largest matching start wins.
constexpr int SPEC_DRAFT_THREADS = 256;
__global__ __launch_bounds__(SPEC_DRAFT_THREADS) void spec_draft_kernel(SpecDraftArgs p) {
    __shared__ int best;
    const int b = blockIdx.x, tid = threadIdx.x, Q = p.Q;
    const int* rs = p.rows + (size_t)b * RS_STRIDE;
    const int step = rs[RS_STEP], max_new = rs[RS_MAXNEW];
    int* tok = p.tok + (size_t)b * Q;
    const int pad = (rs[RS_PAD] >= 0 && rs[RS_PAD] < p.V) ? rs[RS_PAD] : 0;
    const bool live = rs[RS_ACTIVE] && !rs[RS_FINISHED] && step >= 1 && step < max_new;
    if (!live) {   // a finished or full row: no queries; its token rows embed pad so that everything stays finite
        if (tid < Q) tok[tid] = pad;
        if (tid == 0) p.nq[b] = 0;
        return;
    }
    const int L = p.lookup != nullptr ? p.lookup_len[b] : 0, T = p.prompt_len != nullptr ? p.prompt_len[b] : p.prompt_stride;
    const int* lk = p.lookup != nullptr ? p.lookup + (size_t)b * p.lookup_stride : nullptr;
    const int* pr = p.prompt + (size_t)b * p.prompt_stride;
    const int* out = p.out_ids + rs[RS_OUT_OFF];
    const int N = L + 1 + T + step;
    // corpus entry i (i != L: the separator is never read — windows that would cover it are not compared)
    auto at = [&](int i) { return i < L ? lk[i] : (i < L + 1 + T ? pr[i - L - 1] : out[i - L - 1 - T]); };
    int start = -1, ngram = 0;
    for (int ng = min(p.max_ngram, T + step); ng >= 1 && start < 0; --ng) {
        if (tid == 0) best = -1;
        __syncthreads();
        int mine = -1;
        for (int s = tid; s < N - ng; s += SPEC_DRAFT_THREADS) {
            if (s <= L && s + ng > L) continue;   // the window would cover the separator
            bool ok = true;
            for (int i = 0; i < ng && ok; ++i) ok = at(s + i) == at(N - ng + i);
            if (ok) mine = s;
        }
        if (mine >= 0) {
#ifdef VC_EMU
            __atomic_fetch_max(&best, mine, __ATOMIC_RELAXED);
#else
            atomicMax(&best, mine);
#endif
        }
        __syncthreads();
        start = best;
        ngram = ng;
        __syncthreads();
    }
    if (tid != 0) return;
    const int room = min(min(p.k, Q - 1), max_new - step - 1);   // a row with one token left drafts nothing
    int n = 0;
    tok[0] = out[step - 1];   // the last emitted id
    if (start >= 0) {
        for (int i = start + ngram; n < room && i < N && i != L; ++i) {
            const int d = at(i);
            if (d < 0 || d >= p.V) break;
            tok[1 + n++] = d;
        }
    }
    for (int j = 1 + n; j < Q; ++j) tok[j] = pad;
    p.nq[b] = 1 + n;
}
void launch_spec_draft(const SpecDraftArgs& a, hipStream_t s) {
    VC_LAUNCH(spec_draft_kernel, dim3((unsigned)a.B), dim3(SPEC_DRAFT_THREADS), 0, s, a);
}

// Behind the lm_head over the B * Q rows: a_j = greedy argmax of row j (ties to the lower id, as select_embed_kernel); n = the leading
// drafts d_j == a_(j-1); a_0 .. a_n go one by one through emit_token, the plain selection's own bookkeeping, so a finishing token or
// the row's last slot cuts the rest; RS_STEP and RS_POS advance by the number emitted; the last emitted id is the next step's first
// token.  With log-probs, the emitted rows' entries of the scratch a launch_topk_logprob over the B * Q rows filled (entry 0 of a row
// is its argmax) are copied into the slabs.  counters [B][4] += {1, emitted, drafted, emitted - 1}.
// sel != nullptr: a_j = sel[b * Q + j], what spec_select_kernel chose for the row (sampling, processed rows) — nothing is reduced here.
// scratch_chosen != nullptr: the log-prob of a_j is scratch_chosen[b * Q + j] (a sampled token is not entry 0 of its top-K row).
__global__ __launch_bounds__(1024) void spec_accept_kernel(SpecAcceptArgs p) {
    __shared__ BlockRed red;
    __shared__ int a_s[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Q = p.Q;
    const int nq = min(p.nq[b], min(Q, 8));
    if (nq <= 0) return;
    int* rs = p.rows + (size_t)b * RS_STRIDE;
    for (int j = 0; j < nq && p.sel == nullptr; ++j) {
        const float* lg = p.logits + ((size_t)b * Q + j) * p.ldl;
        float best = -INFINITY;
        int bi = 0x7FFFFFFF;
        for (int i = tid * 4; i < p.V; i += 4096) {
            const f32x4 v = ld16f(lg + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) argmax_combine2(best, bi, v[e], i + e);
        }
        block_argmax(best, bi, red, lane, wave);
        if (tid == 0) a_s[j] = bi;
    }
    __syncthreads();
    if (tid != 0) return;
    if (p.sel != nullptr)
        for (int j = 0; j < nq; ++j) a_s[j] = p.sel[(size_t)b * Q + j];
    const int* tok = p.tok + (size_t)b * Q;
    int* out = p.out_ids + rs[RS_OUT_OFF];
    const int max_new = rs[RS_MAXNEW];
    int emitted = 0, last = tok[0];
    for (int j = 0; j < nq; ++j) {
        if (j > 0 && tok[j] != a_s[j - 1]) break;   // draft j is not what the model says behind its predecessors
        const int step = rs[RS_STEP];
        last = emit_token(rs, out, step, a_s[j]);
        if (p.lp_tok != nullptr && step < max_new) {
            const size_t slot = (size_t)rs[RS_OUT_OFF] + step, src = ((size_t)b * Q + j) * p.scratch_k;
            p.lp_tok[slot] = p.scratch_chosen != nullptr ? p.scratch_chosen[(size_t)b * Q + j] : p.scratch_lp[src];
            for (int t = 0; t < p.lp_k; ++t) {
                p.lp_top[slot * p.lp_k + t] = p.scratch_lp[src + t];
                p.lp_ids[slot * p.lp_k + t] = p.scratch_ids[src + t];
            }
        }
        rs[RS_STEP] = step + 1;
        rs[RS_POS] += 1;
        emitted += 1;
        if (rs[RS_FINISHED] || step + 1 >= max_new) break;
    }
    p.next_tok[b] = last;
    if (p.counters != nullptr) {
        int* c = p.counters + 4 * b;
        c[0] += 1;
        c[1] += emitted;
        c[2] += nq - 1;
        c[3] += emitted - 1;
    }
}
void launch_spec_accept(const SpecAcceptArgs& a, hipStream_t s) {
    VC_LAUNCH(spec_accept_kernel, dim3((unsigned)a.B), dim3(1024), 0, s, a);
}

}  // namespace vc
