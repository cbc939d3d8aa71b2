// gemm.hip — bf16 MFMA GEMM for gfx950 with fused epilogues.
//
//   out[m][n] = epilogue( sum_k A[m][k] * W[n][k] + bias[n] )      A:[M,K] bf16, W:[N,K] bf16 (HF Linear layout)
//
// Replaces the torch nn.Linear / Conv2d-as-GEMM calls the reference makes through HF
// ([HF] clip/modeling_clip.py:309-311,333,346-350,
//  [HF] llama/modeling_llama.py:174-176,254-256,280; vcoder_llava/model/multimodal_projector/builder.py:42-46).
//
// Design (CDNA4): 128x128 output tile per 256-thread workgroup (4 waves, 2x2, 64x64 each = 4x4 MFMA
// 16x16x32 fragments, 64 fp32 accumulators per lane), BK=64, two LDS stages (64 KiB -> 2 workgroups/CU),
// XOR-swizzled LDS rows so the ds_read_b128 fragment reads are bank-conflict free, operands staged by LDS-DMA
// (global_load_lds_dwordx4).  Large problems take the 256x256 8-phase kernel below instead.
// The WEIGHT tile is the MFMA A operand and the ACTIVATION tile the B operand, so each lane ends up with
// 4 consecutive output features of one token: epilogues (bias, GELU, residual add, SwiGLU) are lane-local
// and stores are 8/16 bytes per lane.

#include "vc_device.h"
#include <algorithm>
#include <atomic>
#include <stdexcept>

#include "kernels.h"

namespace vc {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * BK * 2;  // one operand tile: 128 rows x 128 B

// byte offset of 16-byte chunk `c` (0..7) of row `r` inside a swizzled [128][64] bf16 tile
VC_DEV int swz(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// map linear workgroup id -> (tile_m, tile_n): XCD-contiguous remap (block b runs on XCD b%8; give each
// XCD a contiguous range of tiles so neighbours share operand panels in that XCD's L2), then groups of
// 8 m-tiles sweep n so a group re-uses its activation panel while streaming weights.
VC_DEV int xcd_remap(int bid, int nblk) {
    const int q = nblk / 8, r = nblk % 8, x = bid % 8, i = bid / 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}
VC_DEV void tile_from_pid(int pid, int tiles_m, int tiles_n, int& tm, int& tn, int GROUP = 8) {
    const int per_group = GROUP * tiles_n;
    const int g = pid / per_group;
    const int first_m = g * GROUP;
    const int gsz = min(tiles_m - first_m, GROUP);
    tm = first_m + (pid % per_group) % gsz;
    tn = (pid % per_group) / gsz;
}
VC_DEV void tile_coords(int bid, int nblk, int tiles_m, int tiles_n, int& tm, int& tn) {
    tile_from_pid(xcd_remap(bid, nblk), tiles_m, tiles_n, tm, tn);
}

// epilogue store of out[m][n..n+3] (shared by all kernels).  p.split_out != 0 (precision mode "split"):
// a bf16 output becomes TWO bf16 planes, hi = bf16(v) at column n and lo = bf16(v - hi) at column split_out + n of the same
// row — the K-concatenated [hi | lo] operand of the next GEMM, which contracts it against the weight matrix twice
// (GemmArgs::kwrap), i.e. with ~16 mantissa bits of the activation instead of 8.
VC_DEV u32x2 pack_bf4(f32x4 v) { return u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])}; }
VC_DEV f32x4 bf4_residual(f32x4 v, u32x2 hi) {
    return f32x4{v[0] - bf2f_lo(hi[0]), v[1] - bf2f_hi(hi[0]), v[2] - bf2f_lo(hi[1]), v[3] - bf2f_hi(hi[1])};
}
// FIX: the caller is the split-K fix-up kernel (a wave = one output row, 4 adjacent lanes = one 16-column tile) instead of an
// MFMA accumulator layout (lanes l, l ^ 16, l ^ 32, l ^ 48 = the 16 columns of one token)
// (the consumer side of the folded RMSNorm — GemmArgs::row_scale — is applied by the callers, which hold a row's scale in a
// register across the columns they store)
// `resid` (EPI_RESID_F32): the residual values out[m][n..n+3] when the caller requested them ahead of time (the 8-phase kernel's
// epilogue: a load inside the caller's bounds guard is waited for with vmcnt(0) at the end of the guard, one round trip per store)
template <int EPI, bool FIX = false>
VC_DEV void store_out(const GemmArgs& p, int m, int n, f32x4 v, const f32x4* resid = nullptr, const f32x4* xgw = nullptr) {
    if constexpr (EPI == EPI_BF16 || EPI == EPI_BF16_QGELU || EPI == EPI_BF16_GELU) {
        if constexpr (EPI == EPI_BF16_QGELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = quick_gelu(v[e]);
        }
        if constexpr (EPI == EPI_BF16_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = erf_gelu(v[e]);
        }
        const u32x2 o = pack_bf4(v);
        bf16_t* dst = reinterpret_cast<bf16_t*>(p.out) + (size_t)m * p.ldo + n;
        st8(dst, o);
        if (p.split_out) st8(dst + p.split_out, pack_bf4(bf4_residual(v, o)));
    } else if constexpr (EPI == EPI_F32) {
        st16f(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + n, v);
    } else if constexpr (EPI == EPI_RESID_F32) {
        float* o = reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + n;
        v = (resid != nullptr ? *resid : ld16f(o)) + v;
        st16f(o, v);
        if (p.xg_out) {   // folded RMSNorm, producer side: the next GEMM's operand and the row's sum-of-squares partial
            const f32x4 t = v * (xgw != nullptr ? *xgw : ld16f(p.xg_w + n));
            const u32x2 hi = pack_bf4(t);
            bf16_t* d = p.xg_out + (size_t)m * p.ld_xg + n;
            st8(d, hi);
            if (p.xg_lo) st8(d + p.xg_lo, pack_bf4(bf4_residual(t, hi)));
            float sq = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
            // the 16 columns of the tile sit in 4 lanes that share this lane's m (so they are all here: N % 16 == 0)
            if constexpr (FIX) {
                sq += shfl_xor(sq, 1);
                sq += shfl_xor(sq, 2);
            } else {
                sq = rows_sum(sq);
            }
            if (FIX ? (lane_id() & 3) == 0 : lane_id() < 16) p.ssq_out[(size_t)m * p.npart + (n >> 4)] = sq;
        }
    } else {  // EPI_SWIGLU: (g0,u0,g1,u1) -> 2 outputs
        const float h0 = silu(v[0]) * v[1], h1 = silu(v[2]) * v[3];
        const uint32_t o = pack_bf2(h0, h1);
        bf16_t* dst = reinterpret_cast<bf16_t*>(p.out) + (size_t)m * p.ldo + (n >> 1);
        *reinterpret_cast<uint32_t*>(dst) = o;
        if (p.split_out) *reinterpret_cast<uint32_t*>(dst + p.split_out) = pack_bf2(h0 - bf2f_lo(o), h1 - bf2f_hi(o));
    }
}

// byte offset of the WEIGHT operand's k-tile (128 bytes = 64 bf16) for k-tile `kt` of the contraction: with GemmArgs::kwrap =
// K_w / BK the weight matrix is contracted against both halves of a K-concatenated [hi | lo] activation row (K = 2 K_w), i.e. its
// k index wraps; with GemmArgs::w_lo_off a third segment (k-tiles [2 kwrap, 3 kwrap)) takes the weight's lo plane against the
// activation's hi plane (a_koff: the activation's k index wraps back to 0 there)
VC_DEV long long w_koff(int kt, const GemmArgs& p) {
    if (p.kwrap <= 0 || kt < p.kwrap) return (long long)kt * 128;
    if (kt < 2 * p.kwrap) return (long long)(kt - p.kwrap) * 128;
    return p.w_lo_off + (long long)(kt - 2 * p.kwrap) * 128;
}
VC_DEV long long a_koff(int kt, const GemmArgs& p) {
    return (long long)((p.kwrap > 0 && kt >= 2 * p.kwrap) ? kt - 2 * p.kwrap : kt) * 128;
}


// ---- EPI_QKV (kernels.h QkvEpiArgs): RoPE + head split + KV write in the QKV GEMM's epilogue ---------------------------------
// weight row behind row `row` (0..127) of X half `h` of the 256-row tile at n0: {head 2a: d 0..63 | head 2a+1: d 0..63} in half 0,
// the same heads' d 64..127 in half 1 — wave group g = row / 64 then owns ONE head in both halves
VC_DEV int qkv_wrow(int n0, int h, int row) { return n0 + (row >> 6) * 128 + h * 64 + (row & 63); }
// A row behind padded token row mp = b * Tp + t (clamped into the sample; the stores of such rows are masked)
VC_DEV int qkv_arow(const QkvEpiArgs& e, int mp) {
    const int b = min(mp / e.Tp, e.B - 1);
    return b * e.T + min(mp - b * e.Tp, e.T - 1);
}
// 4 rotate-half pairs (x = d0 + i, y = d0 + 64 + i) of token (b, t), head `head`: the projection is rounded to bf16 first (the value
// the unfused path stores in its fused rows), RoPE in fp32 on the rounded values (rope_pair, the split kernel's own function), rounded
// again; which = 0: Q rows, 1: K rows (+ the e4m3 cache row)
// cs / sn: rope_cos / rope_sin [t][dl .. dl + 3] (the GEMM's epilogue requests them ahead of its bounds guards)
VC_DEV void qkv_rope_store(const QkvEpiArgs& e, int which, int head, int b, int t, int dl, f32x4 x, f32x4 y, f32x4 cs, f32x4 sn) {
    const u32x2 xb = pack_bf4(x), yb = pack_bf4(y);
    u32x2 olo, ohi;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
        const float x0 = bf2f_lo(xb[h2]), x1 = bf2f_hi(xb[h2]), y0 = bf2f_lo(yb[h2]), y1 = bf2f_hi(yb[h2]);
        const float c0 = cs[2 * h2], c1 = cs[2 * h2 + 1], s0 = sn[2 * h2], s1 = sn[2 * h2 + 1];
        float a0, b0, a1, b1;
        rope_pair(x0, y0, c0, s0, a0, b0);
        rope_pair(x1, y1, c1, s1, a1, b1);
        olo[h2] = pack_bf2(a0, a1);
        ohi[h2] = pack_bf2(b0, b1);
    }
    const size_t bh = (size_t)b * e.H + head;
    bf16_t* dst = which == 0 ? e.q + (bh * e.q_stride + t) * 128 : e.k + (bh * e.kv_stride + t) * 128;
    st8(dst + dl, olo);
    st8(dst + 64 + dl, ohi);
    if (which == 1 && e.k8 != nullptr) {
        uint8_t* d8 = e.k8 + (bh * e.kv8_stride + t) * 128;
        *reinterpret_cast<uint32_t*>(d8 + dl) = f32x4_to_fp8x4(bf2f_lo(olo[0]), bf2f_hi(olo[0]), bf2f_lo(olo[1]), bf2f_hi(olo[1]));
        *reinterpret_cast<uint32_t*>(d8 + 64 + dl) = f32x4_to_fp8x4(bf2f_lo(ohi[0]), bf2f_hi(ohi[0]), bf2f_lo(ohi[1]), bf2f_hi(ohi[1]));
    }
}
VC_DEV void qkv_rope_store(const QkvEpiArgs& e, int which, int head, int b, int t, int dl, f32x4 x, f32x4 y) {
    qkv_rope_store(e, which, head, b, t, dl, x, y, ld16f(e.rope_cos + (size_t)t * 64 + dl), ld16f(e.rope_sin + (size_t)t * 64 + dl));
}
// 4 value features d0 .. d0 + 3 of token (b, t) into the cache row(s)
VC_DEV void qkv_v_store(const QkvEpiArgs& e, int head, int b, int t, int d0, u32x2 vb) {
    const size_t bh = (size_t)b * e.H + head;
    if (e.v != nullptr) st8(e.v + (bh * e.kv_stride + t) * 128 + d0, vb);
    if (e.v8 != nullptr)
        *reinterpret_cast<uint32_t*>(e.v8 + (bh * e.kv8_stride + t) * 128 + d0) =
            f32x4_to_fp8x4(bf2f_lo(vb[0]), bf2f_hi(vb[0]), bf2f_lo(vb[1]), bf2f_hi(vb[1]));
}
// column of key kk (0..31) of a 32-key block inside the V^T scratch row (attn.hip vt_chunk_key0: chunk c holds keys 4c..4c+3, 16+4c..16+4c+3)
VC_DEV int vt_pos32(int kk) { return ((kk & 15) >> 2) * 8 + (kk & 3) + 4 * (kk >> 4); }

// ---- LDS-DMA staging: the next k-tile is copied global->LDS by global_load_lds_dwordx4 (no staging VGPRs, no ds_write_b128)
// while the MFMAs of the current tile run; the compiler's vmcnt(0) before the tile's closing barrier retires it.  One
// wave-instruction fills 8 swizzled rows (1 KiB): lane p writes slot p%8 of row p/8, so it FETCHES chunk (p%8)^(row&7) of that row.
// Geometry: WN x WM waves, each owning FI x FJ MFMA tiles (16 features x 16 tokens) -> workgroup tile
// BNt = WN*FI*16 features x BMt = WM*FJ*16 tokens.  <2,2,4,4> = 128x128 / 4 waves / 64 KiB LDS (2 workgroups per CU).
template <int EPI, int WN, int WM, int FI, int FJ>
__global__ __launch_bounds__(WN * WM * 64) void gemm_bf16_dma_kernel(GemmArgs p) {
    constexpr int BNt = WN * FI * 16, BMt = WM * FJ * 16, NW = WN * WM;
    constexpr int W_BYTES = BNt * 128, A_BYTES = BMt * 128, STAGE = W_BYTES + A_BYTES;
    constexpr int WP = BNt / 8 / NW, AP = BMt / 8 / NW;  // 1-KiB DMA pieces per wave per operand tile
    VC_DYNAMIC_SMEM(char, smem);  // [2 stages][W tile | A tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave / WM, wm = wave % WM;
    const int tiles_m = (p.M + BMt - 1) / BMt, tiles_n = (p.N + BNt - 1) / BNt;
    int tm, tn;
    tile_coords(blockIdx.x, tiles_m * tiles_n, tiles_m, tiles_n, tm, tn);
    const int m0 = tm * BMt, n0 = tn * BNt;
    const char* a_src[AP];
    const char* w_src[WP];
    // a 1-KiB piece = 8 swizzled rows; lane p fills slot p%8 of row p/8, i.e. fetches chunk (p%8)^(row&7) of that row
#pragma unroll
    for (int i = 0; i < WP; ++i) {
        const int row = (i * NW + wave) * 8 + (lane >> 3);
        const int wr = min(n0 + row, p.N - 1);
        w_src[i] = reinterpret_cast<const char*>(p.W + (size_t)wr * p.ldw) + (((lane & 7) ^ (row & 7)) << 4);
    }
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int row = (i * NW + wave) * 8 + (lane >> 3);
        const int am = min(m0 + row, p.M - 1);
        a_src[i] = reinterpret_cast<const char*>(p.A + (size_t)am * p.lda) + (((lane & 7) ^ (row & 7)) << 4);
    }
    auto issue_tile = [&](int kt, int stage) {
        char* ws = smem + stage * STAGE;
        char* as = ws + W_BYTES;
#pragma unroll
        for (int i = 0; i < WP; ++i) glds16(w_src[i] + w_koff(kt, p), ws + (i * NW + wave) * 1024);
#pragma unroll
        for (int i = 0; i < AP; ++i) glds16(a_src[i] + a_koff(kt, p), as + (i * NW + wave) * 1024);
    };
    f32x4 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = p.K / BK;
    issue_tile(0, 0);
    __syncthreads();
    const int frow = lane & 15, fchunk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) issue_tile(kt + 1, (kt + 1) & 1);
        const char* ws = smem + (kt & 1) * STAGE;
        const char* as = ws + W_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 fw[FI], fa[FJ];
#pragma unroll
            for (int i = 0; i < FI; ++i) fw[i] = ld16(ws + swz(wn * (FI * 16) + i * 16 + frow, ks * 4 + fchunk));
#pragma unroll
            for (int j = 0; j < FJ; ++j) fa[j] = ld16(as + swz(wm * (FJ * 16) + j * 16 + frow, ks * 4 + fchunk));
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) acc[i][j] = mfma16(fw[i], fa[j], acc[i][j]);
        }
        __syncthreads();
    }

    // ---- epilogue: lane holds out[m][n..n+3], m = .. + (lane&15), n = .. + (lane>>4)*4
#pragma unroll
    for (int i = 0; i < FI; ++i) {
        const int n = n0 + wn * (FI * 16) + i * 16 + (lane >> 4) * 4;
        if (n >= p.N) continue;
        f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.bias) bv = ld16f(p.bias + n);
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const int m = m0 + wm * (FJ * 16) + j * 16 + (lane & 15);
            if (m >= p.M) continue;
            store_out<EPI>(p, m, n, (p.row_scale ? acc[i][j] * p.row_scale[m] : acc[i][j]) + bv);
        }
    }
}


// ---- 256 x 256 tile, 8 waves, counted-vmcnt "8-phase" schedule ----------------------------------------------------------
// The one-barrier loop above drains the LDS-DMA queue (vmcnt(0)) at every k-tile barrier, so HBM/L2 latency is exposed
// once per tile.  Here the DMA stream runs 3 half-tiles ahead and is never drained inside the loop:
//   * a k-tile (BK = 64) is staged as four 16-KiB half-tiles  Y0 | X0 | Y1 | X1  (X = weight rows n, Y = activation rows
//     m; half h = tile rows [128h, 128h+128)), double-buffered: 2 x 64 KiB;
//   * wave (g, q) = (wave/4, wave%4) owns n rows {64g..64g+63} of BOTH X halves and m rows {32q..32q+31} of BOTH Y halves,
//     i.e. a 128 x 64 output made of four 64 x 32 quadrants; one quadrant x BK = 16 MFMAs = one phase;
//   * phase r of k-tile t:  r=0 reads Y0,X0 (12 fragments) and stages X1(t+1);  r=1 reads Y1, stages Y0(t+2);
//     r=2 reads X1, stages X0(t+2);  r=3 reads nothing, stages Y1(t+2) and waits vmcnt(6) — everything except the three
//     most recent half-tiles has landed, which is exactly k-tile t+1.  Every restage targets a half-tile whose last
//     fragment read retired at least one full barrier earlier (Y0: lgkmcnt(8) before the r=0 barrier);
//   * the two wave groups g = 0/1 (the two waves of every SIMD) run one barrier apart, so one group's 16 MFMAs (under
//     s_setprio 1) overlap the other group's fragment reads + DMA issue; barriers are bare s_barrier.
// LDS-DMA data is ordered for a ds_read only by the issuing wave's vmcnt wait followed by a barrier the reader passes;
// the r=3 wait precedes that phase's first barrier and the first read of the retired buffer is a phase later.
//
// F8 = true: the same schedule over OCP e4m3 operands (activations quantised per token row, weights per output row, both
// with power-of-two scales): a 128-byte tile row is now ONE K = 128 step of v_mfma_scale_f32_16x16x128_f8f6f4 (unit
// block scales; twice the bf16 MFMA rate) instead of two K = 32 bf16 steps — identical bytes, LDS layout, DMA pattern
// and MFMA cycles per k-tile, half the k-tiles.  A lane feeds the instruction chunks g and 4+g of its row (g = lane/16) —
// the fragment reads of the bf16 form, which are bank-conflict free; reading the "natural" chunks 2g, 2g+1 measured 50 %
// conflict cycles.  Which 32 of the row's 128 k a lane contributes is free as long as both operands agree: the
// instruction sums over all of them.  The epilogue multiplies the fp32 accumulator by a_scale[m] * w_scale[n] (exact: powers of two).
// KWRAP (precision mode "split"): the weight's k-tile index wraps after p.kwrap tiles (compile-time flag: the default
// instantiation keeps the weight source a plain `base + kt * 128`, exactly the round-2 loop)
template <int EPI, bool F8 = false, bool KWRAP = false>
__global__ __launch_bounds__(512) void gemm_bf16_8phase_kernel(GemmArgs p) {
    static_assert(!(EPI == EPI_QKV && KWRAP), "the fused QKV epilogue has no K-wrapped form");
    constexpr int HALF = 128 * 128, TILE = 4 * HALF;  // bytes
    constexpr int ES = F8 ? 1 : 2;                    // bytes per operand element; a k-tile is 128 bytes of every row
    constexpr int SY0 = 0, SX0 = HALF, SY1 = 2 * HALF, SX1 = 3 * HALF;
    VC_DYNAMIC_SMEM(char, smem);  // [2][Y0 | X0 | Y1 | X1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = wave >> 2, q = wave & 3;
    const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
    // split-K remainder round: workgroups [sk_full, ...) are sk_ks K-slices of each of the last tiles
    int pid, ks = 0, KS = 1;
    if (p.sk_ks > 1 && (int)blockIdx.x >= p.sk_full) {
        const int r = (int)blockIdx.x - p.sk_full;
        pid = p.sk_full + r / p.sk_ks;
        ks = r % p.sk_ks;
        KS = p.sk_ks;
    } else {
        pid = p.xcd_remap_on ? xcd_remap(blockIdx.x, p.sk_ks > 1 ? p.sk_full : tiles_m * tiles_n) : (int)blockIdx.x;
    }
    int tm, tn;
    tile_from_pid(pid, tiles_m, tiles_n, tm, tn, p.tile_group);
    const int m0 = tm * 256, n0 = tn * 256;
    const int nk_all = p.K * ES / 128;
    const int kt_first = (int)((long)ks * nk_all / KS);
    // DMA sources: every wave moves pieces {wave, 8 + wave} (8 swizzled rows = 1 KiB each) of every half-tile
    const char* x_src[2][2];
    const char* y_src[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (i * 8 + wave) * 8 + (lane >> 3);
            const int sw = ((lane & 7) ^ (row & 7)) << 4;
            const int wrow = EPI == EPI_QKV ? qkv_wrow(n0, h, row) : n0 + h * 128 + row;
            int arow = min(m0 + h * 128 + row, p.M - 1);
            if constexpr (EPI == EPI_QKV) arow = qkv_arow(p.qe, arow);
            x_src[h][i] = reinterpret_cast<const char*>(p.W) + (size_t)min(wrow, p.N - 1) * p.ldw * ES + sw +
                          (KWRAP ? (size_t)0 : (size_t)kt_first * 128);
            y_src[h][i] = reinterpret_cast<const char*>(p.A) + (size_t)arow * p.lda * ES + sw +
                          (KWRAP ? (size_t)0 : (size_t)kt_first * 128);
        }
    const int nk = (int)((long)(ks + 1) * nk_all / KS) - kt_first;  // k-tiles of this workgroup
    auto stage_x = [&](int h, int kt) {
        if (kt >= nk) return;
        char* dst = smem + (kt & 1) * TILE + (h ? SX1 : SX0) + wave * 1024;
        const long long wk = KWRAP ? w_koff(kt_first + kt, p) : (long long)kt * 128;
        glds16(x_src[h][0] + wk, dst);
        glds16(x_src[h][1] + wk, dst + 8192);
    };
    auto stage_y = [&](int h, int kt) {
        if (kt >= nk) return;
        char* dst = smem + (kt & 1) * TILE + (h ? SY1 : SY0) + wave * 1024;
        const long long ak = KWRAP ? a_koff(kt_first + kt, p) : (long long)kt * 128;
        glds16(y_src[h][0] + ak, dst);
        glds16(y_src[h][1] + ak, dst + 8192);
    };
    f32x4 acc[2][4][2][2];  // [x half][i][y half][j]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[a][i][b][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fchunk = lane >> 4;
    // X0 is dead after phase 1 and X1 is first read in phase 2: one register set serves both halves
    u32x4 fx[4][2], fy[2][2][2];  // [fragment][ks], [half][fragment][ks]
    auto read_x = [&](const char* base, int h) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                fx[i][ks] = ld16(base + (h ? SX1 : SX0) + swz(g * 64 + i * 16 + frow, ks * 4 + fchunk));
    };
    auto read_y = [&](const char* base, int h) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                fy[h][j][ks] = ld16(base + (h ? SY1 : SY0) + swz(q * 32 + j * 16 + frow, ks * 4 + fchunk));
    };
    auto quadrant = [&](int hx, int hy) {
        set_prio<1>();
        if constexpr (F8) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[hx][i][hy][j] = mfma16_f8(fx[i][0], fx[i][1], fy[hy][j][0], fy[hy][j][1], acc[hx][i][hy][j]);
            // the scaled-MFMA intrinsic is sunk by the optimiser (all 32 of a k-tile end up behind the loop's last barrier,
            // out of their s_setprio brackets) unless its results are pinned here
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) pin_vgprs(acc[hx][i][hy][j]);
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[hx][i][hy][j] = mfma16(fx[i][ks], fy[hy][j][ks], acc[hx][i][hy][j]);
        }
        set_prio<0>();
    };
    // prologue: k-tile 0 complete, the first three half-tiles of k-tile 1 in flight
    stage_y(0, 0); stage_x(0, 0); stage_y(1, 0); stage_x(1, 0);
    stage_y(0, 1); stage_x(0, 1); stage_y(1, 1);
    if (nk > 1) wait_vmcnt<6>();
    else wait_vmcnt<0>();
    wg_barrier_raw();
    if (g == 1) wg_barrier_raw();  // group 1 runs one barrier behind group 0
    for (int kt = 0; kt < nk; ++kt) {
        const char* base = smem + (kt & 1) * TILE;
        // r = 0
        read_y(base, 0);
        sched_fence();
        read_x(base, 0);
        stage_x(1, kt + 1);
        wait_lgkmcnt<8>();  // the Y0 reads (issued first) have retired: Y0 may be restaged next phase
        wg_barrier_raw();
        wait_lgkmcnt<0>();
        quadrant(0, 0);
        wg_barrier_raw();
        // r = 1
        read_y(base, 1);
        stage_y(0, kt + 2);
        wg_barrier_raw();
        wait_lgkmcnt<0>();
        quadrant(0, 1);
        wg_barrier_raw();
        // r = 2
        read_x(base, 1);
        stage_x(0, kt + 2);
        wg_barrier_raw();
        wait_lgkmcnt<0>();
        quadrant(1, 1);
        wg_barrier_raw();
        // r = 3
        stage_y(1, kt + 2);
        if (kt + 2 < nk) wait_vmcnt<6>();  // all of k-tile kt+1 has landed (3 newer half-tiles may be in flight)
        else wait_vmcnt<0>();
        wg_barrier_raw();
        quadrant(1, 0);
        wg_barrier_raw();
    }
    if (g == 0) wg_barrier_raw();

    if (KS > 1) {  // partial tile -> workspace [remainder tile][slice][256 m][256 n]; the fix-up launch finishes it
        float* base = p.ws + ((size_t)(pid - p.sk_full) * KS + ks) * 65536;
#pragma unroll
        for (int hx = 0; hx < 2; ++hx)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        st16f(base + (hy * 128 + q * 32 + j * 16 + (lane & 15)) * 256 + hx * 128 + g * 64 + i * 16 + (lane >> 4) * 4,
                              acc[hx][i][hy][j]);
        return;
    }
    if constexpr (EPI == EPI_QKV) {
        // lane holds, for its wave group's head, features d = hx * 64 + i * 16 + G * 4 + (0..3) of tokens hy * 128 + q * 32 + j * 16 + l15
        const QkvEpiArgs& e = p.qe;
        const int D = e.H * 128;
        const int which = n0 / D, head = (n0 - which * D) / 128 + g;
        const int G = lane >> 4, l15 = lane & 15;
        int tb[2][2], tt[2][2];
        bool ok[2][2];
        float rs[2][2];
#pragma unroll
        for (int hy = 0; hy < 2; ++hy)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int mp = m0 + hy * 128 + q * 32 + j * 16 + l15;
                tb[hy][j] = mp / e.Tp;
                tt[hy][j] = mp - tb[hy][j] * e.Tp;
                ok[hy][j] = mp < p.M && tt[hy][j] < e.T;
                const int src = qkv_arow(e, min(mp, p.M - 1));
                rs[hy][j] = F8 ? p.a_scale[src] : (p.row_scale ? p.row_scale[src] : 1.f);
            }
        if (which < 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int dl = i * 16 + G * 4, nx = n0 + g * 128 + dl;   // nx: the weight row (= output column) of x; y is 64 further
                f32x4 bx = f32x4{0.f, 0.f, 0.f, 0.f}, by = bx, swx = f32x4{1.f, 1.f, 1.f, 1.f}, swy = swx;
                if (p.bias) {
                    bx = ld16f(p.bias + nx);
                    by = ld16f(p.bias + nx + 64);
                }
                if constexpr (F8) {
                    swx = ld16f(p.w_scale + nx);
                    swy = ld16f(p.w_scale + nx + 64);
                }
                // the cos / sin rows of the lane's four tokens: requested together at a clamped token and waited for OUTSIDE the
                // guards (round 6, as the RESID epilogue below: inside the guard every store paid its own table round trip and the
                // drain of the stores before it)
                f32x4 csv[2][2], snv[2][2];
#pragma unroll
                for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const size_t tc = (size_t)min(tt[hy][j], e.T - 1) * 64 + dl;
                        csv[hy][j] = ld16f(e.rope_cos + tc);
                        snv[hy][j] = ld16f(e.rope_sin + tc);
                    }
#pragma unroll
                for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        pin_vgprs(csv[hy][j]);
                        pin_vgprs(snv[hy][j]);
                    }
                pin_vgprs(bx);
                pin_vgprs(by);
                if constexpr (F8) {
                    pin_vgprs(swx);
                    pin_vgprs(swy);
                }
#pragma unroll
                for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        if (ok[hy][j])
                            qkv_rope_store(e, which, head, tb[hy][j], tt[hy][j], dl, acc[0][i][hy][j] * (swx * rs[hy][j]) + bx,
                                           acc[1][i][hy][j] * (swy * rs[hy][j]) + by, csv[hy][j], snv[hy][j]);
            }
        } else {
#pragma unroll
            for (int hx = 0; hx < 2; ++hx)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d0 = hx * 64 + i * 16 + G * 4, nv = n0 + g * 128 + d0;
                    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f}, sw = f32x4{1.f, 1.f, 1.f, 1.f};
                    if (p.bias) bv = ld16f(p.bias + nv);
                    if constexpr (F8) sw = ld16f(p.w_scale + nv);
                    pin_vgprs(bv);
                    if constexpr (F8) pin_vgprs(sw);
#pragma unroll
                    for (int hy = 0; hy < 2; ++hy) {
                        u32x2 vb[2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            vb[j] = pack_bf4(acc[hx][i][hy][j] * (sw * rs[hy][j]) + bv);
                            if (ok[hy][j]) qkv_v_store(e, head, tb[hy][j], tt[hy][j], d0, vb[j]);
                            else vb[j] = u32x2{0u, 0u};   // keys behind the sequence are zeros in the V^T scratch
                        }
                        // P[f] = feature d0 + f of the lane's two tokens (keys kk = l15 and 16 + l15 of the 32-key block); after the
                        // quad transpose lane r = l15 & 3 holds feature d0 + r of keys 4c .. 4c + 3 and 16 + 4c .. 16 + 4c + 3
                        // (c = l15 >> 2): chunk c of the block in the flash kernel's key order — one 16-byte store
                        uint32_t P[4] = {(vb[0][0] & 0xFFFFu) | (vb[1][0] << 16), (vb[0][0] >> 16) | (vb[1][0] & 0xFFFF0000u),
                                         (vb[0][1] & 0xFFFFu) | (vb[1][1] << 16), (vb[0][1] >> 16) | (vb[1][1] & 0xFFFF0000u)};
                        quad_transpose4(P, l15 & 3);
                        const int base = m0 + hy * 128 + q * 32, bb = base / e.Tp, t0 = base - bb * e.Tp, c = l15 >> 2;
                        if (base < p.M && t0 + 4 * c < e.T)
                            st16(e.vt + (((size_t)bb * e.H + head) * 128 + d0 + (l15 & 3)) * e.vt_stride + t0 + 8 * c,
                                 u32x4{(P[0] & 0xFFFFu) | (P[1] << 16), (P[2] & 0xFFFFu) | (P[3] << 16), (P[0] >> 16) | (P[1] & 0xFFFF0000u),
                                       (P[2] >> 16) | (P[3] & 0xFFFF0000u)});
                    }
                }
        }
        return;
    }
    // ---- epilogue: lane holds out[m][n..n+3]
    float rsc[2][2] = {{1.f, 1.f}, {1.f, 1.f}};   // folded RMSNorm, consumer side: the row scales of this lane's four token rows
    if (p.row_scale) {
#pragma unroll
        for (int hy = 0; hy < 2; ++hy)
#pragma unroll
            for (int j = 0; j < 2; ++j) rsc[hy][j] = p.row_scale[min(m0 + hy * 128 + q * 32 + j * 16 + (lane & 15), p.M - 1)];
    }
    // Everything the stores need from memory is requested AHEAD of the bounds guards, unconditionally at clamped addresses and in
    // batches (round 6, ISA): a load inside a guard is waited for with vmcnt(0) where the guard ends, so the RESID epilogue of
    // rounds 1-5 paid 32 DEPENDENT residual round trips per lane (a quarter of the o_proj launch: MFMA-busy 49 % where the other
    // epilogues' kernels show 60-67 %), the bias / weight-scale loads 8.  Now: the column operands of a tile half together, the
    // residual values of two column groups (8 loads) together.
    float asc[2][2] = {{1.f, 1.f}, {1.f, 1.f}};   // W8A8: the activation rows' scales
    if constexpr (F8) {
#pragma unroll
        for (int hy = 0; hy < 2; ++hy)
#pragma unroll
            for (int j = 0; j < 2; ++j) asc[hy][j] = p.a_scale[min(m0 + hy * 128 + q * 32 + j * 16 + (lane & 15), p.M - 1)];
    }
#pragma unroll
    for (int hx = 0; hx < 2; ++hx) {
        f32x4 bvh[4], swh[4], gwh[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nc = min(n0 + hx * 128 + g * 64 + i * 16 + (lane >> 4) * 4, p.N - 4);
            bvh[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            swh[i] = f32x4{1.f, 1.f, 1.f, 1.f};
            if (p.bias) bvh[i] = ld16f(p.bias + nc);          // (wave-uniform test: the four loads of the half go out together)
            if constexpr (F8) swh[i] = ld16f(p.w_scale + nc);
            if constexpr (EPI == EPI_RESID_F32) {             // folded-RMSNorm producer: the consumer's norm weights of these columns
                gwh[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (p.xg_out) gwh[i] = ld16f(p.xg_w + nc);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pin_vgprs(bvh[i]);
            if constexpr (F8) pin_vgprs(swh[i]);
            if constexpr (EPI == EPI_RESID_F32) pin_vgprs(gwh[i]);
        }
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            f32x4 res[2][2][2];
            if constexpr (EPI == EPI_RESID_F32) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int nc = min(n0 + hx * 128 + g * 64 + (ip * 2 + ii) * 16 + (lane >> 4) * 4, p.N - 4);
                            const int mc = min(m0 + hy * 128 + q * 32 + j * 16 + (lane & 15), p.M - 1);
                            res[ii][hy][j] = ld16f(reinterpret_cast<const float*>(p.out) + (size_t)mc * p.ldo + nc);
                        }
                // ... and waited for HERE, outside the guards (an empty asm that takes the registers): a first use inside a guard
                // leaves them pending on the path around it, and every later guarded use then drains the stores issued since
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                        for (int j = 0; j < 2; ++j) pin_vgprs(res[ii][hy][j]);
            }
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = ip * 2 + ii;
                const int n = n0 + hx * 128 + g * 64 + i * 16 + (lane >> 4) * 4;
                if (n >= p.N) continue;
#pragma unroll
                for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int m = m0 + hy * 128 + q * 32 + j * 16 + (lane & 15);
                        if (m >= p.M) continue;
                        if constexpr (EPI == EPI_QKV) {
                        } else if constexpr (F8) store_out<EPI>(p, m, n, acc[hx][i][hy][j] * (swh[i] * asc[hy][j]) + bvh[i]);
                        else if constexpr (EPI == EPI_RESID_F32) store_out<EPI>(p, m, n, acc[hx][i][hy][j] * rsc[hy][j] + bvh[i], &res[ii][hy][j], &gwh[i]);
                        else store_out<EPI>(p, m, n, acc[hx][i][hy][j] * rsc[hy][j] + bvh[i]);
                    }
            }
        }
    }
}

// sums the K-slices of the split remainder tiles in k order and applies the epilogue (one thread = out[m][n..n+3])
template <int EPI>
__global__ __launch_bounds__(256) void gemm_splitk_fixup_kernel(GemmArgs p) {
    const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
    const int r = blockIdx.x >> 6;
    const int idx = ((int)(blockIdx.x & 63) << 8) + threadIdx.x;
    const int ml = idx >> 6, nl = (idx & 63) << 2;
    int tm, tn;
    tile_from_pid(p.sk_full + r, tiles_m, tiles_n, tm, tn, p.tile_group);
    const int m = tm * 256 + ml, n = tn * 256 + nl;
    if (m >= p.M || n >= p.N) return;
    const float* base = p.ws + (size_t)r * p.sk_ks * 65536 + ml * 256 + nl;
    f32x4 v = ld16f(base);
    for (int k = 1; k < p.sk_ks; ++k) v = v + ld16f(base + (size_t)k * 65536);
    if (p.f8) v = v * (ld16f(p.w_scale + n) * p.a_scale[m]);
    if (p.row_scale) v = v * p.row_scale[m];
    if (p.bias) v = v + ld16f(p.bias + n);
    store_out<EPI, true>(p, m, n, v);
}


// ... and of the fused-QKV epilogue: one thread = the rotate-half pairs (x at tile column c, y at column 128 + c) of 4 features of
// one token of a remainder tile; V^T elements are stored one by one here (a few remainder tiles per launch)
__global__ __launch_bounds__(256) void gemm_splitk_fixup_qkv_kernel(GemmArgs p) {
    const QkvEpiArgs& e = p.qe;
    const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
    const int r = blockIdx.x >> 5;
    const int idx = ((int)(blockIdx.x & 31) << 8) + threadIdx.x;
    const int ml = idx >> 5, cx = (idx & 31) << 2;   // cx: tile column of x (0..124) = g * 64 + dl
    int tm, tn;
    tile_from_pid(p.sk_full + r, tiles_m, tiles_n, tm, tn, p.tile_group);
    const int mp = tm * 256 + ml, n0 = tn * 256;
    const int b = mp / e.Tp, t = mp - b * e.Tp;
    if (mp >= p.M || t >= e.T) return;
    const float* base = p.ws + (size_t)r * p.sk_ks * 65536 + ml * 256 + cx;
    f32x4 x = ld16f(base), y = ld16f(base + 128);
    for (int k = 1; k < p.sk_ks; ++k) {
        x = x + ld16f(base + (size_t)k * 65536);
        y = y + ld16f(base + (size_t)k * 65536 + 128);
    }
    const int D = e.H * 128, which = n0 / D, g = cx >> 6, dl = cx & 63, head = (n0 - which * D) / 128 + g, nx = n0 + g * 128 + dl;
    const int src = b * e.T + t;
    if (p.f8) {
        x = x * (ld16f(p.w_scale + nx) * p.a_scale[src]);
        y = y * (ld16f(p.w_scale + nx + 64) * p.a_scale[src]);
    }
    if (p.row_scale) {
        x = x * p.row_scale[src];
        y = y * p.row_scale[src];
    }
    if (p.bias) {
        x = x + ld16f(p.bias + nx);
        y = y + ld16f(p.bias + nx + 64);
    }
    if (which < 2) {
        qkv_rope_store(e, which, head, b, t, dl, x, y);
        return;
    }
    const u32x2 vx = pack_bf4(x), vy = pack_bf4(y);
    qkv_v_store(e, head, b, t, dl, vx);
    qkv_v_store(e, head, b, t, 64 + dl, vy);
    bf16_t* vt = e.vt + (((size_t)b * e.H + head) * 128) * e.vt_stride + (t & ~31) + vt_pos32(t & 31);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        vt[(size_t)(dl + f) * e.vt_stride] = (bf16_t)(f & 1 ? vx[f >> 1] >> 16 : vx[f >> 1] & 0xFFFFu);
        vt[(size_t)(64 + dl + f) * e.vt_stride] = (bf16_t)(f & 1 ? vy[f >> 1] >> 16 : vy[f >> 1] & 0xFFFFu);
    }
    if (t == e.T - 1)   // the keys behind the sequence inside its last 32-key block are zeros (as the tile epilogue writes them)
        for (int kk = (t & 31) + 1; kk < 32; ++kk)
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                e.vt[(((size_t)b * e.H + head) * 128 + dl + f) * e.vt_stride + (t & ~31) + vt_pos32(kk)] = 0;
                e.vt[(((size_t)b * e.H + head) * 128 + 64 + dl + f) * e.vt_stride + (t & ~31) + vt_pos32(kk)] = 0;
            }
}

// rstd of every row from the sum-of-squares partials a RESID epilogue published (one wave per row, fixed order)
__global__ __launch_bounds__(256) void rstd_from_partials_kernel(const float* ssq, int npart, int nparts, float* rstd, int rows, int D,
                                                                 float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int i = lane; i < nparts; i += 64) s += ssq[(size_t)row * npart + i];
    s = wave_sum(s);
    if (lane == 0) rstd[row] = rsqrtf(s / (float)D + eps);
}
void launch_rstd_from_partials(const float* ssq, int npart, int nparts, float* rstd, int rows, int D, float eps, hipStream_t s) {
    VC_LAUNCH(rstd_from_partials_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, ssq, npart, nparts, rstd, rows, D, eps);
}

// The 8-phase kernel over 256 x 256 tiles, and the fix-up of its split-K remainder round.  Tile order: 4 m-tiles per sweep group
// (measured: 4 and 2 beat 8 / 16 / 38 by 2-6 %) and the XCD remap on (+-3 %).  Split-K for a short last round: the rem <= 128
// tiles left over after the full rounds of 256 are cut into ks = 256 / rem K-slices each (at most 8, at most one per k-tile of
// 128 bytes, within the workspace), so the round is ~1/ks as long; a.ws == nullptr (vc_model_set_batch_invariant) keeps it whole.
template <int EPI, bool F8, bool KWRAP = false>
static void launch_gemm_8phase(const GemmArgs& a, hipStream_t s) {
    constexpr size_t lds = 2 * (256 * 128 + 256 * 128);
    const long t256 = (long)((a.M + 255) / 256) * ((a.N + 255) / 256), rem = t256 % 256;
    GemmArgs ask = a;
    ask.tile_group = 4;
    ask.xcd_remap_on = 1;
    ask.sk_full = (int)t256;
    ask.sk_ks = 1;
    if (a.ws && t256 > 256 && rem > 0 && rem <= 128) {
        int ks = (int)std::min<long>(256 / rem, 8);
        ks = std::min(ks, a.K / (F8 ? 128 : BK));
        while (ks > 1 && (size_t)rem * ks * 65536 * 4 > a.ws_bytes) --ks;
        if (ks > 1) {
            ask.sk_full = (int)(t256 - rem);
            ask.sk_ks = ks;
        }
    }
#ifndef VC_EMU
    static const hipError_t lds_set = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_8phase_kernel<EPI, F8, KWRAP>),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   // once per kernel
    (void)lds_set;
#endif
    const dim3 grid((unsigned)(ask.sk_ks > 1 ? ask.sk_full + rem * ask.sk_ks : t256));
    VC_LAUNCH((gemm_bf16_8phase_kernel<EPI, F8, KWRAP>), grid, dim3(512), lds, s, ask);
    if (ask.sk_ks == 1) return;
    if constexpr (EPI == EPI_QKV) VC_LAUNCH(gemm_splitk_fixup_qkv_kernel, dim3((unsigned)(rem * 32)), dim3(256), 0, s, ask);
    else VC_LAUNCH((gemm_splitk_fixup_kernel<EPI>), dim3((unsigned)(rem * 64)), dim3(256), 0, s, ask);
}

// test hook (vck_set_gemm_force_8phase): the bf16 8-phase kernel for every size inside one process
static bool g_force_8phase = false;
void set_gemm_force_8phase(bool on) { g_force_8phase = on; }
// which kernel launch_gemm chose, counted on the host (tests pin the dispatch rule to the shapes they mean to cover)
static std::atomic<unsigned long> g_gemm_dma_launches{0}, g_gemm_8phase_launches{0};   // sessions launch from their own threads
unsigned long gemm_dma_launches() { return g_gemm_dma_launches.load(std::memory_order_relaxed); }
unsigned long gemm_8phase_launches() { return g_gemm_8phase_launches.load(std::memory_order_relaxed); }

// The e4m3 form (GemmArgs::f8) and the fused QKV epilogue always take the 8-phase kernel (any size: rows are clamped, stores
// masked); the other bf16 GEMMs take it from M >= 1024 and N >= 512 on, the 128 x 128 LDS-DMA kernel below that.
void launch_gemm(const GemmArgs& a, int epilogue, hipStream_t s) {
    if (a.xg_out && (epilogue != EPI_RESID_F32 || a.N % 16 != 0 || !a.xg_w || !a.ssq_out || a.npart < a.N / 16))
        throw std::runtime_error("gemm: the folded-RMSNorm producer needs EPI_RESID_F32, N % 16 == 0, xg_w, ssq_out, npart >= N / 16");
    if (epilogue == EPI_QKV) {
        const QkvEpiArgs& e = a.qe;
        if (a.kwrap > 0 || a.xg_out || e.H <= 0 || (e.H * 128) % 256 != 0 || a.N != 3 * e.H * 128 || e.Tp % 32 != 0 || e.Tp < e.T ||
            a.M != e.B * e.Tp || !e.q || !e.k || !e.vt || !e.rope_cos || !e.rope_sin || (!e.v && !e.v8))
            throw std::runtime_error("gemm: EPI_QKV needs hd 128, D % 256 == 0, N = 3 D, M = B * Tp with Tp = rup(T, 32), q / k / v / vt and the RoPE tables");
    }
    const bool eight = a.f8 || epilogue == EPI_QKV || g_force_8phase || (a.M >= 1024 && a.N >= 512);
    (eight ? g_gemm_8phase_launches : g_gemm_dma_launches).fetch_add(1, std::memory_order_relaxed);
    if (a.f8) {
        switch (epilogue) {
            case EPI_QKV: return launch_gemm_8phase<EPI_QKV, true>(a, s);
            case EPI_BF16: return launch_gemm_8phase<EPI_BF16, true>(a, s);
            case EPI_RESID_F32: return launch_gemm_8phase<EPI_RESID_F32, true>(a, s);
            case EPI_SWIGLU: return launch_gemm_8phase<EPI_SWIGLU, true>(a, s);
            default: throw std::runtime_error("fp8 GEMM: epilogue not instantiated");
        }
    }
    if (epilogue == EPI_QKV) return launch_gemm_8phase<EPI_QKV, false>(a, s);
    if (eight) {
#define VC_G8(E) return a.kwrap > 0 ? launch_gemm_8phase<E, false, true>(a, s) : launch_gemm_8phase<E, false>(a, s)
        switch (epilogue) {
            case EPI_BF16: VC_G8(EPI_BF16);
            case EPI_BF16_QGELU: VC_G8(EPI_BF16_QGELU);
            case EPI_BF16_GELU: VC_G8(EPI_BF16_GELU);
            case EPI_F32: VC_G8(EPI_F32);
            case EPI_RESID_F32: VC_G8(EPI_RESID_F32);
            default: VC_G8(EPI_SWIGLU);
        }
#undef VC_G8
    }
    const dim3 grid(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN)), block(256);
    const size_t shmem = 4 * TILE_BYTES;
    switch (epilogue) {
        case EPI_BF16: VC_LAUNCH((gemm_bf16_dma_kernel<EPI_BF16, 2, 2, 4, 4>), grid, block, shmem, s, a); break;
        case EPI_BF16_QGELU: VC_LAUNCH((gemm_bf16_dma_kernel<EPI_BF16_QGELU, 2, 2, 4, 4>), grid, block, shmem, s, a); break;
        case EPI_BF16_GELU: VC_LAUNCH((gemm_bf16_dma_kernel<EPI_BF16_GELU, 2, 2, 4, 4>), grid, block, shmem, s, a); break;
        case EPI_F32: VC_LAUNCH((gemm_bf16_dma_kernel<EPI_F32, 2, 2, 4, 4>), grid, block, shmem, s, a); break;
        case EPI_RESID_F32: VC_LAUNCH((gemm_bf16_dma_kernel<EPI_RESID_F32, 2, 2, 4, 4>), grid, block, shmem, s, a); break;
        default: VC_LAUNCH((gemm_bf16_dma_kernel<EPI_SWIGLU, 2, 2, 4, 4>), grid, block, shmem, s, a); break;
    }
}

}  // namespace vc
