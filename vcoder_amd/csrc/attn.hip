// attn.hip — attention for the VCoder hot path on gfx950.
//
//   qkv_split   : fused-QKV GEMM output -> Q [B,H,Tq,hd], K cache [B,H,S,hd], V^T scratch [B,H,hd,S] in the flash kernel's
//                 key order (vt_chunk_key0 below) (+RoPE)
//                 RoPE = rotate_half form of [HF] llama/modeling_llama.py:113-160 (cos/sin fp32 table)      K13/K14
//   attention   : flash-style softmax(Q K^T * scale [+causal]) V, fp32 online softmax, MFMA 16x16x32 bf16
//                 ViT: [HF] clip/modeling_clip.py:259-277,320-330 (non-causal, hd 64, T 577)              K5
//                 LLM prefill: [HF] llama eager_attention_forward :191-214 (causal, hd 128)               K15
//   attention_decode : q_len = 1 over the KV cache (HBM-streaming, VALU dot products)                    K15
//
// Layout choices are ours (the reference has none): K is key-major so K tiles are MFMA A-operands for
// S^T = K Q^T straight from LDS; V is stored TRANSPOSED (d-major) so V^T tiles are A-operands for
// O^T = V^T P^T; with S^T in the MFMA C layout each lane already owns the P values of ONE query, so
// row max / row sum need only 2 cross-lane steps and P feeds the second MFMA from registers (the
// contraction order over keys is permuted identically on both operands).

#include <stdexcept>
#include <type_traits>

#include "vc_device.h"
#include "kernels.h"

namespace vc {

// Key order of the V^T scratch (the flash kernel's A operand of O^T = V^T P^T).  Inside every aligned block of 32 keys the
// 16-byte chunk c (0..3) of a row holds keys {4c..4c+3, 16+4c..16+4c+3}: position 8c + e <-> key 4c + (e & 3) + 16 (e >> 2)
// (vt_key_pos in tests/kernel_cases.py).  That is the order in which the S^T accumulators of a lane (MFMA C layout: sub-tile
// `sub`, lane group g, register r <-> key 16 sub + 4g + r) are packed into the P operand, so a lane's 8 contraction values of
// a 32-key half are one contiguous chunk.  The scratch is written and read only by the kernels of this file.
VC_DEV int vt_chunk_key0(int chunk_in_tile) { return (chunk_in_tile >> 2) * 32 + (chunk_in_tile & 3) * 4; }

// =============================================================================================
// qkv split (+RoPE), prefill form: one workgroup = (64-token tile, head, batch)
// =============================================================================================
template <int HD>
__global__ __launch_bounds__(256) void qkv_split_kernel(QkvSplitArgs p) {
    const float* __restrict__ rope_cos = p.rope_cos;
    const float* __restrict__ rope_sin = p.rope_sin;
    __shared__ __attribute__((aligned(16))) bf16_t vt_tile[64][HD + 8];  // +8 bf16 pad: transposed reads spread banks
    const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int D = p.H * HD;
    constexpr int CPT = HD / 16;  // rope work items per token: chunk c pairs d0=8c with d0+HD/2
    const bool rope = rope_cos != nullptr;
    for (int w = tid; w < 64 * CPT; w += 256) {
        const int tl = w / CPT, c = w % CPT, t = t0 + tl;
        if (t >= p.T) continue;
        const bf16_t* row = p.qkv + ((size_t)b * p.T + t) * (3 * D) + h * HD;
#pragma unroll
        for (int which = 0; which < 2; ++which) {  // 0 = q, 1 = k
            const bf16_t* src = row + which * D;
            const u32x4 lo = ld16(src + c * 8), hi = ld16(src + HD / 2 + c * 8);
            u32x4 olo = lo, ohi = hi;
            if (rope) {
                const float* cs = rope_cos + (size_t)t * (HD / 2) + c * 8;
                const float* sn = rope_sin + (size_t)t * (HD / 2) + c * 8;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x0 = bf2f_lo(lo[e]), x1 = bf2f_hi(lo[e]), y0 = bf2f_lo(hi[e]), y1 = bf2f_hi(hi[e]);
                    const float c0 = cs[2 * e], c1 = cs[2 * e + 1], s0 = sn[2 * e], s1 = sn[2 * e + 1];
                    float a0, b0, a1, b1;   // out[d] = x*cos - y*sin ; out[d+hd/2] = y*cos + x*sin
                    rope_pair(x0, y0, c0, s0, a0, b0);
                    rope_pair(x1, y1, c1, s1, a1, b1);
                    olo[e] = pack_bf2(a0, a1);
                    ohi[e] = pack_bf2(b0, b1);
                }
            }
            bf16_t* dst = which == 0 ? p.q + (((size_t)b * p.H + h) * p.q_stride + t) * HD
                                     : p.k + (((size_t)b * p.H + h) * p.kv_stride + t) * HD;
            st16(dst + c * 8, olo);
            st16(dst + HD / 2 + c * 8, ohi);
            if (which == 1 && p.k8 != nullptr) {   // e4m3 cache row: the bf16 values above, re-rounded
                uint8_t* d8 = p.k8 + (((size_t)b * p.H + h) * p.kv8_stride + t) * HD;
                st8(d8 + c * 8, u32x2{f32x4_to_fp8x4(bf2f_lo(olo[0]), bf2f_hi(olo[0]), bf2f_lo(olo[1]), bf2f_hi(olo[1])),
                                      f32x4_to_fp8x4(bf2f_lo(olo[2]), bf2f_hi(olo[2]), bf2f_lo(olo[3]), bf2f_hi(olo[3]))});
                st8(d8 + HD / 2 + c * 8, u32x2{f32x4_to_fp8x4(bf2f_lo(ohi[0]), bf2f_hi(ohi[0]), bf2f_lo(ohi[1]), bf2f_hi(ohi[1])),
                                               f32x4_to_fp8x4(bf2f_lo(ohi[2]), bf2f_hi(ohi[2]), bf2f_lo(ohi[3]), bf2f_hi(ohi[3]))});
            }
        }
    }
    // V: rows as they are into the cache (key-major, what the decode steps stream); and a staged [token][d] tile written
    // back as V^T rows, 16 bytes (8 tokens) at a time, for the flash kernel of THIS prefill / ViT layer
    const int vts = p.vt_stride > 0 ? p.vt_stride : p.kv_stride;
    for (int w = tid; w < 64 * (HD / 8); w += 256) {
        const int tl = w / (HD / 8), c = w % (HD / 8), t = t0 + tl;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (t < p.T) {
            v = ld16(p.qkv + ((size_t)b * p.T + t) * (3 * D) + 2 * D + h * HD + c * 8);
            if (p.v != nullptr) st16(p.v + (((size_t)b * p.H + h) * p.kv_stride + t) * HD + c * 8, v);
            if (p.v8 != nullptr)
                st8(p.v8 + (((size_t)b * p.H + h) * p.kv8_stride + t) * HD + c * 8,
                    u32x2{f32x4_to_fp8x4(bf2f_lo(v[0]), bf2f_hi(v[0]), bf2f_lo(v[1]), bf2f_hi(v[1])),
                          f32x4_to_fp8x4(bf2f_lo(v[2]), bf2f_hi(v[2]), bf2f_lo(v[3]), bf2f_hi(v[3]))});
        }
        st16(&vt_tile[tl][c * 8], v);
    }
    __syncthreads();
    for (int w = tid; w < HD * 8; w += 256) {
        const int d = w >> 3, tc = w & 7;
        const int k0 = vt_chunk_key0(tc);      // chunk tc of the tile holds keys k0..k0+3 and k0+16..k0+19 (vt_key_pos)
        if (t0 + k0 >= p.T) continue;
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = k0 + (e >> 1) * 16 + (e & 1) * 2;
            o[e] = (uint32_t)vt_tile[key][d] | ((uint32_t)vt_tile[key + 1][d] << 16);
        }
        st16(p.vt + (((size_t)b * p.H + h) * HD + d) * vts + t0 + tc * 8, u32x4{o[0], o[1], o[2], o[3]});
    }
}

// ---- precision mode "split": fp32 projection output -> RoPE in fp32 -> (i) the fp32 K / V cache rows the decode steps read,
// (ii) bf16 hi / lo planes of Q, K and V^T for the MFMA flash kernel of THIS prefill / ViT layer (x = hi + lo to ~16 bits)
VC_DEV void split8(const float* v, u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hi[e] = pack_bf2(v[2 * e], v[2 * e + 1]);
        lo[e] = pack_bf2(v[2 * e] - bf2f_lo(hi[e]), v[2 * e + 1] - bf2f_hi(hi[e]));
    }
}
template <int HD>
__global__ __launch_bounds__(256) void qkv_split32_kernel(QkvSplit32Args p) {
    const float* __restrict__ rope_cos = p.rope_cos;
    const float* __restrict__ rope_sin = p.rope_sin;
    __shared__ __attribute__((aligned(16))) bf16_t vt_tile[2][64][HD + 8];  // [hi / lo][token][d]
    const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x;
    const int D = p.H * HD;
    constexpr int CPT = HD / 16;  // rope work items per token: chunk c pairs d0 = 8c with d0 + HD/2
    const bool rope = rope_cos != nullptr;
    const size_t bh = (size_t)b * p.H + h;
    for (int w = tid; w < 64 * CPT; w += 256) {
        const int tl = w / CPT, c = w % CPT, t = t0 + tl;
        if (t >= p.T) continue;
        const float* row = p.qkv + ((size_t)b * p.T + t) * (3 * D) + h * HD;
#pragma unroll
        for (int which = 0; which < 2; ++which) {  // 0 = q, 1 = k
            const float* src = row + which * D;
            float x[8], y[8], ox[8], oy[8];
            *reinterpret_cast<f32x4*>(x) = ld16f(src + c * 8);
            *reinterpret_cast<f32x4*>(x + 4) = ld16f(src + c * 8 + 4);
            *reinterpret_cast<f32x4*>(y) = ld16f(src + HD / 2 + c * 8);
            *reinterpret_cast<f32x4*>(y + 4) = ld16f(src + HD / 2 + c * 8 + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float cs = 1.f, sn = 0.f;
                if (rope) {
                    cs = rope_cos[(size_t)t * (HD / 2) + c * 8 + e];
                    sn = rope_sin[(size_t)t * (HD / 2) + c * 8 + e];
                }
                ox[e] = x[e] * cs - y[e] * sn;   // out[d] = x*cos - y*sin ; out[d+hd/2] = y*cos + x*sin
                oy[e] = y[e] * cs + x[e] * sn;
            }
            u32x4 xh, xl, yh, yl;
            split8(ox, xh, xl);
            split8(oy, yh, yl);
            const size_t off = which == 0 ? (bh * p.q_stride + t) * HD : (bh * p.ks_stride + t) * HD;
            bf16_t* dh = (which == 0 ? p.q_hi : p.k_hi) + off;
            bf16_t* dl = (which == 0 ? p.q_lo : p.k_lo) + off;
            st16(dh + c * 8, xh);
            st16(dl + c * 8, xl);
            st16(dh + HD / 2 + c * 8, yh);
            st16(dl + HD / 2 + c * 8, yl);
            if (which == 1 && p.k32 != nullptr) {
                if (p.kv24) {   // fp24 cache row: hd x u16 hi plane | hd x u8 lo plane
                    char* kc = reinterpret_cast<char*>(p.k32) + (bh * p.kv_stride + t) * (size_t)(3 * HD);
                    u32x4 h8;
                    u32x2 l8;
                    pack_f24x8(ox, h8, l8);
                    st16(kc + c * 16, h8);
                    st8(kc + 2 * HD + c * 8, l8);
                    pack_f24x8(oy, h8, l8);
                    st16(kc + HD + c * 16, h8);
                    st8(kc + 2 * HD + HD / 2 + c * 8, l8);
                } else {
                    float* kc = p.k32 + (bh * p.kv_stride + t) * HD;
                    st16f(kc + c * 8, *reinterpret_cast<f32x4*>(ox));
                    st16f(kc + c * 8 + 4, *reinterpret_cast<f32x4*>(ox + 4));
                    st16f(kc + HD / 2 + c * 8, *reinterpret_cast<f32x4*>(oy));
                    st16f(kc + HD / 2 + c * 8 + 4, *reinterpret_cast<f32x4*>(oy + 4));
                }
            }
        }
    }
    for (int w = tid; w < 64 * (HD / 8); w += 256) {
        const int tl = w / (HD / 8), c = w % (HD / 8), t = t0 + tl;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (t < p.T) {
            const float* src = p.qkv + ((size_t)b * p.T + t) * (3 * D) + 2 * D + h * HD + c * 8;
            *reinterpret_cast<f32x4*>(v) = ld16f(src);
            *reinterpret_cast<f32x4*>(v + 4) = ld16f(src + 4);
            if (p.v32 != nullptr) {
                if (p.kv24) {
                    char* vc = reinterpret_cast<char*>(p.v32) + (bh * p.kv_stride + t) * (size_t)(3 * HD);
                    u32x4 h8;
                    u32x2 l8;
                    pack_f24x8(v, h8, l8);
                    st16(vc + c * 16, h8);
                    st8(vc + 2 * HD + c * 8, l8);
                } else {
                    float* vc = p.v32 + (bh * p.kv_stride + t) * HD + c * 8;
                    st16f(vc, *reinterpret_cast<f32x4*>(v));
                    st16f(vc + 4, *reinterpret_cast<f32x4*>(v + 4));
                }
            }
        }
        u32x4 vh, vl;
        split8(v, vh, vl);
        st16(&vt_tile[0][tl][c * 8], vh);
        st16(&vt_tile[1][tl][c * 8], vl);
    }
    __syncthreads();
    for (int w = tid; w < 2 * HD * 8; w += 256) {
        const int pl = w / (HD * 8), d = (w >> 3) % HD, tc = w & 7;
        const int k0 = vt_chunk_key0(tc);
        if (t0 + k0 >= p.T) continue;
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = k0 + (e >> 1) * 16 + (e & 1) * 2;
            o[e] = (uint32_t)vt_tile[pl][key][d] | ((uint32_t)vt_tile[pl][key + 1][d] << 16);
        }
        st16((pl ? p.vt_lo : p.vt_hi) + (bh * HD + d) * p.vt_stride + t0 + tc * 8, u32x4{o[0], o[1], o[2], o[3]});
    }
}
void launch_qkv_split32(const QkvSplit32Args& a, hipStream_t s) {
    const dim3 grid((a.T + 63) / 64, a.H, a.B), block(256);
    if (a.hd == 128) VC_LAUNCH((qkv_split32_kernel<128>), grid, block, 0, s, a);
    else VC_LAUNCH((qkv_split32_kernel<64>), grid, block, 0, s, a);
}

void launch_qkv_split(const QkvSplitArgs& a, hipStream_t s) {
    const dim3 grid((a.T + 63) / 64, a.H, a.B), block(256);
    if (a.hd == 128) VC_LAUNCH((qkv_split_kernel<128>), grid, block, 0, s, a);
    else VC_LAUNCH((qkv_split_kernel<64>), grid, block, 0, s, a);
}

// =============================================================================================
// flash attention: workgroup = 128 queries of one (b,h) as WAVES waves x QS 16-query sub-tiles; KV tiles of 64 keys
// =============================================================================================
template <int HD> VC_DEV int swz_k(int row, int chunk) {  // K tile [64][HD] bf16, 16-B chunks
    if constexpr (HD == 128) return row * 256 + ((chunk ^ (row & 15)) << 4);
    else return row * 128 + ((chunk ^ (row & 7)) << 4);
}
VC_DEV int swz_v(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }  // V^T tile [HD][64]

// SPLIT (precision mode "split"): every operand comes as two bf16 planes (x = hi + lo, ~16 mantissa bits): S^T = Kh Qh + Kh Ql
// + Kl Qh, the softmax numerators are split the same way in registers, O^T += Vh Ph + Vh Pl + Vl Ph (the lo x lo terms are
// below 2^-18 relative), and the output row is written as [hi | lo] at columns h*HD and lo_off + h*HD of a row of ldo
// elements.  Twice the LDS per stage (dynamic shared memory: 128 KiB at hd 128, one workgroup per CU).
template <int HD, bool CAUSAL, int WAVES, int QS, bool SPLIT = false>
__global__ __launch_bounds__(WAVES * 64, (WAVES == 8 && QS == 1 && !SPLIT) ? 4 : 1) void attention_kernel(AttnArgs p) {  // 8 x 16: two workgroups per CU (<= 128 VGPRs)
    constexpr int NTH = WAVES * 64;       // threads per workgroup
    constexpr int QB = WAVES * QS * 16;   // queries per workgroup
    constexpr int KS = HD / 32;        // k-steps of the QK^T contraction
    constexpr int DT = HD / 16;        // 16-wide d tiles of the output
    constexpr int KCH = HD / 8;        // 16-B chunks per K row
    constexpr int KB_ = 64 * HD * 2, VB_ = HD * 128;   // bytes of a K tile [64 keys][HD] and a V^T tile [HD][64 keys]
    constexpr int PL = SPLIT ? 2 : 1;                  // operand planes
    constexpr int STAGE = PL * (KB_ + VB_);            // [K hi | K lo | V^T hi | V^T lo]
    char* lds0;                                        // [2][STAGE], double-buffered: the LDS-DMA of tile t+1 lands under tile t
#ifdef VC_EMU   // the emulator's guard page, NaN poison and race check cover DYNAMIC LDS: the test build takes both forms from it
    VC_DYNAMIC_SMEM(char, lds_dyn);
    lds0 = lds_dyn;
#else
    if constexpr (SPLIT) {
        VC_DYNAMIC_SMEM(char, lds_dyn);
        lds0 = lds_dyn;
    } else {
        __shared__ __attribute__((aligned(16))) char lds_st[2 * STAGE];
        lds0 = lds_st;
    }
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    // Workgroup order.  sched 0: the 3-D grid as launched (query block fastest).  Otherwise a 1-D grid whose linear id — the
    // hardware hands consecutive ids to consecutive XCDs — is mapped so that (1, 3) every XCD owns a contiguous range of
    // (b, h) pairs: the query blocks of a head run on ONE XCD and its K / V^T tiles are fetched into that L2 once, not into
    // eight; and (1, 2) the query blocks of a causal pass are taken heaviest first (block i has ~2 (i + 1) KV tiles), so the
    // launch ends on the light ones instead of a few 19-tile stragglers.
    int qb_ = blockIdx.x, h_ = blockIdx.y, b_ = blockIdx.z;
    if (p.sched != 0) {
        const int lin = blockIdx.x, BH = p.B * p.H;
        int head, qr;
        if (p.sched == 2) {
            head = lin % BH;
            qr = lin / BH;
        } else {
            const int xcd = lin & 7, r = lin >> 3, per = BH >> 3;   // the launcher checks BH % 8 == 0
            head = xcd * per + r / p.nqb;
            qr = r % p.nqb;
        }
        qb_ = (CAUSAL && p.sched != 3) ? p.nqb - 1 - qr : qr;
        h_ = head % p.H;
        b_ = head / p.H;
    }
    const int q0 = qb_ * QB, h = h_, b = b_;
    const size_t bh = (size_t)b * p.H + h;
    const bf16_t* qbase = p.q + bh * p.q_stride * HD;
    const bf16_t* kbase = p.k + bh * p.kv_stride * HD;
    const int vts = p.vt_stride > 0 ? p.vt_stride : p.kv_stride;
    const bf16_t* vbase = p.vt + bh * HD * (size_t)vts;
    const bf16_t* qbase_lo = SPLIT ? p.q_lo + bh * p.q_stride * HD : nullptr;
    const bf16_t* kbase_lo = SPLIT ? p.k_lo + bh * p.kv_stride * HD : nullptr;
    const bf16_t* vbase_lo = SPLIT ? p.vt_lo + bh * HD * (size_t)vts : nullptr;

    // Q fragments (MFMA B operand): lane holds Q[query j][d = ks*32 + g*8 .. +8]
    u32x4 qf[QS][KS], qfl[SPLIT ? QS : 1][SPLIT ? KS : 1];
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) {
        const int qrow = min(q0 + wave * (QS * 16) + qs * 16 + j, p.T - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[qs][ks] = ld16(qbase + (size_t)qrow * HD + ks * 32 + g * 8);
            if constexpr (SPLIT) qfl[qs][ks] = ld16(qbase_lo + (size_t)qrow * HD + ks * 32 + g * 8);
        }
    }
    f32x4 o[QS][DT];
#pragma unroll
    for (int qs = 0; qs < QS; ++qs)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[qs][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[QS], l_run[QS];
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) { m_run[qs] = -INFINITY; l_run[qs] = 0.f; }

    const float c2 = p.scale * 1.4426950408889634f;   // scale * log2(e): exp(scale * x) = exp2(c2 * x)
    const int kv_end = CAUSAL ? min(p.T, q0 + QB) : p.T;
    const int nkt = (kv_end + 63) / 64;
    // K / V^T tiles go global -> LDS by DMA (global_load_lds_dwordx4: no staging VGPRs, no ds_write pass), 1-KiB pieces =
    // 64 lanes x 16 B written linearly; the XOR swizzles of swz_k / swz_v are applied on the SOURCE side: the lane that
    // fills slot s of row r fetches chunk s ^ f(r) of that row.
    constexpr int KROWS = 1024 / (HD * 2);      // K rows per piece (4 at hd 128, 8 at hd 64)
    constexpr int KPIECES = KB_ / 1024 / WAVES, VPIECES = VB_ / 1024 / WAVES;
    static_assert(KPIECES >= 1 && VPIECES >= 1 && KB_ % (1024 * WAVES) == 0 && VB_ % (1024 * WAVES) == 0, "pieces per wave");
    const char* ksrc[KPIECES];
    const char* vsrc[VPIECES];
    size_t koff[KPIECES], voff[VPIECES];   // element offsets inside a (b,h) plane: the lo planes share them
#pragma unroll
    for (int i = 0; i < KPIECES; ++i) {
        const int piece = i * WAVES + wave, row = piece * KROWS + lane / KCH, slot = lane % KCH;
        const int ch = HD == 128 ? (slot ^ (row & 15)) : (slot ^ (row & 7));
        koff[i] = (size_t)row * HD + ch * 8;
        ksrc[i] = reinterpret_cast<const char*>(kbase + koff[i]);
    }
#pragma unroll
    for (int i = 0; i < VPIECES; ++i) {
        const int piece = i * WAVES + wave, row = piece * 8 + (lane >> 3), slot = lane & 7;
        voff[i] = (size_t)row * vts + ((slot ^ ((row >> 1) & 7)) * 8);
        vsrc[i] = reinterpret_cast<const char*>(vbase + voff[i]);
    }
    // stage layout: K hi at 0, [K lo at KB_,] V^T hi at PL*KB_, [V^T lo at PL*KB_ + VB_]
    auto issue_tile = [&](int kt, int buf) {
        char* st = lds0 + buf * STAGE;
#pragma unroll
        for (int i = 0; i < KPIECES; ++i) {
            glds16(ksrc[i] + (size_t)kt * (64 * HD * 2), st + (i * WAVES + wave) * 1024);
            if constexpr (SPLIT)
                glds16(reinterpret_cast<const char*>(kbase_lo + koff[i]) + (size_t)kt * (64 * HD * 2), st + KB_ + (i * WAVES + wave) * 1024);
        }
#pragma unroll
        for (int i = 0; i < VPIECES; ++i) {
            glds16(vsrc[i] + (size_t)kt * 128, st + PL * KB_ + (i * WAVES + wave) * 1024);
            if constexpr (SPLIT)
                glds16(reinterpret_cast<const char*>(vbase_lo + voff[i]) + (size_t)kt * 128, st + PL * KB_ + VB_ + (i * WAVES + wave) * 1024);
        }
    };

    const int w_first = q0 + wave * (QS * 16);   // smallest query of this wave
    issue_tile(0, 0);
    for (int kt = 0; kt < nkt; ++kt) {
        // tile kt has landed for every wave (own vmcnt wait + barrier) and every wave is done with tile kt-1, whose buffer
        // the next DMA overwrites
        wait_vmcnt<0>();
        __syncthreads();
        if (kt + 1 < nkt) issue_tile(kt + 1, (kt + 1) & 1);
        const char* k_lds = lds0 + (kt & 1) * STAGE;
        const char* v_lds = k_lds + PL * KB_;
        const int k0 = kt * 64;
        // Tiles this wave has nothing to do in (it still takes part in the DMA and the barrier above): every key of the tile
        // lies in the future of all its queries — the last tile of a causal block for the lower half of its waves — or all
        // its queries lie behind the sequence (the ragged last block: S = 1216 leaves waves 4..7 of block 9, the 19-tile one,
        // without a row).  Together 13 % of the wave-tiles of the prefill shape; the skipped work contributed exact zeros.
        if (w_first >= p.T || (CAUSAL && k0 > w_first + QS * 16 - 1)) continue;
        // ---- S^T = K Q^T
        f32x4 sacc[QS][4];
#pragma unroll
        for (int qs = 0; qs < QS; ++qs)
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) sacc[qs][sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const u32x4 kf = ld16(k_lds + swz_k<HD>(sub * 16 + j, ks * 4 + g));
#pragma unroll
                for (int qs = 0; qs < QS; ++qs) sacc[qs][sub] = mfma16(kf, qf[qs][ks], sacc[qs][sub]);
                if constexpr (SPLIT) {
                    const u32x4 kl = ld16(k_lds + KB_ + swz_k<HD>(sub * 16 + j, ks * 4 + g));
#pragma unroll
                    for (int qs = 0; qs < QS; ++qs) {
                        sacc[qs][sub] = mfma16(kf, qfl[qs][ks], sacc[qs][sub]);
                        sacc[qs][sub] = mfma16(kl, qf[qs][ks], sacc[qs][sub]);
                    }
                }
            }
        // ---- online softmax (lane owns query j of each q-subtile; keys spread over regs and the 4 lane groups).  The
        // kernel is bound by these VALU / transcendental instructions, not by its MFMAs (per query-key pair: 256 MACs =
        // 0.25 MFMA cycles against one v_exp_f32 and the arithmetic around it), so the per-element work is the minimum:
        // the running maximum is kept on the RAW scores (scale > 0 commutes with max), scale * log2(e) is folded into the
        // one FMA that feeds v_exp_f32, and the key mask is only evaluated in tiles that contain a masked key (the
        // diagonal tiles of a causal pass, the ragged last tile) — a wave-uniform branch.
        u32x4 pb[QS][2], pbl[SPLIT ? QS : 1][2];
#pragma unroll
        for (int qs = 0; qs < QS; ++qs) {
            const int qfirst = q0 + wave * (QS * 16) + qs * 16;     // smallest query of this sub-tile
            const int query = qfirst + j;
            if ((CAUSAL && k0 + 63 > qfirst) || k0 + 64 > p.T || p.key_mask != nullptr) {
                // key_mask (padded batches): a key hidden by the caller's attention_mask is hidden from EVERY query of its
                // sequence, exactly as the additive mask HF builds from the 2-D mask ([HF] llama/modeling_llama.py causal mask +
                // padding mask); key 0 of a sequence is always visible (the engine checks), so the running maximum is finite
                const uint8_t* km = p.key_mask != nullptr ? p.key_mask + (size_t)b * p.mask_stride : nullptr;
                if (km == nullptr) {   // the common case: sixteen selects, no branches
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int key = k0 + sub * 16 + g * 4 + r;
                            const bool hide = key >= p.T || (CAUSAL && key > query);
                            sacc[qs][sub][r] = hide ? -INFINITY : sacc[qs][sub][r];
                        }
                } else {
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int key = k0 + sub * 16 + g * 4 + r;
                            if (key >= p.T || (CAUSAL && key > query) || km[key] == 0) sacc[qs][sub][r] = -INFINITY;
                        }
                }
            }
            // v_max3 on the raw accumulators (fmaxf would canonicalise every MFMA output first: 16 extra VALU per tile)
            float mx = vmax3(sacc[qs][0][0], sacc[qs][0][1], sacc[qs][0][2]);
            mx = vmax3(mx, sacc[qs][0][3], sacc[qs][1][0]);
            mx = vmax3(mx, sacc[qs][1][1], sacc[qs][1][2]);
            mx = vmax3(mx, sacc[qs][1][3], sacc[qs][2][0]);
            mx = vmax3(mx, sacc[qs][2][1], sacc[qs][2][2]);
            mx = vmax3(mx, sacc[qs][2][3], sacc[qs][3][0]);
            mx = vmax3(mx, sacc[qs][3][1], sacc[qs][3][2]);
            mx = vmax2(mx, sacc[qs][3][3]);
            mx = rows_max(mx);
            // Deferred maximum: the reference point m of exp(scale * (s - m)) only has to keep the exponentials in range, it
            // need not BE the maximum.  It moves (and O, l are rescaled) only when some query of the sub-tile exceeds it by more
            // than DEFER — a wave-uniform branch that is rarely taken once the first tiles are done; in between P <= e^8, exact
            // in fp32 and with the same relative bf16 rounding.  Precision mode "split" keeps the threshold at 0: the reference
            // point is then the running maximum itself and skipping the no-op rescale (alpha == 1) changes no bit.
            constexpr float DEFER = SPLIT ? 0.f : 11.5f;            // in log2 units: e^8
            const bool grew = wave_any((mx - m_run[qs]) * c2 > DEFER);   // first tile: m_run = -inf
            const float m_new = grew ? vmax2(m_run[qs], mx) : m_run[qs];   // raw-score units; finite from the first tile on (key 0)
            const float alpha = grew ? fast_exp2((m_run[qs] - m_new) * c2) : 1.0f;  // first tile: exp2(-inf) = 0
            m_run[qs] = m_new;
            const float mc = m_new * c2;
            float rs = 0.f;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = fast_exp2(fmaf(sacc[qs][sub][r], c2, -mc));   // = exp(scale * (s - m)); masked: 0
                    sacc[qs][sub][r] = e;
                    rs += e;
                }
            if (grew) {
                l_run[qs] = l_run[qs] * alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[qs][dt] = o[qs][dt] * alpha;
            }
            l_run[qs] += rs;
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
                pb[qs][kh] = u32x4{pack_bf2(sacc[qs][2 * kh][0], sacc[qs][2 * kh][1]),
                                   pack_bf2(sacc[qs][2 * kh][2], sacc[qs][2 * kh][3]),
                                   pack_bf2(sacc[qs][2 * kh + 1][0], sacc[qs][2 * kh + 1][1]),
                                   pack_bf2(sacc[qs][2 * kh + 1][2], sacc[qs][2 * kh + 1][3])};
            if constexpr (SPLIT) {
#pragma unroll
                for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const f32x4& sv = sacc[qs][2 * kh + (e >> 1)];
                        const uint32_t hi = pb[qs][kh][e];
                        pbl[qs][kh][e] = pack_bf2(sv[2 * (e & 1)] - bf2f_lo(hi), sv[2 * (e & 1) + 1] - bf2f_hi(hi));
                    }
            }
        }
        // ---- O^T += V^T P^T   (contraction slot (g,e) <-> key kh*32 + (e>>2)*16 + 4g + (e&3) on both operands: the V^T scratch
        // stores the keys of every 32-key block in exactly that order, so a lane's 8 contraction values are ONE 16-byte chunk —
        // one conflict-free ds_read_b128 per MFMA.  Two 8-byte reads of a key-ordered tile were merged by the compiler into
        // ds_read2st64_b64, which banks mod 32 in contiguous 16-lane groups: 39 % of the kernel's LDS cycles were conflicts)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                const int row = dt * 16 + j;
                const u32x4 vf = ld16(v_lds + swz_v(row, kh * 4 + g));   // keys 32 kh + {4g..4g+3, 16+4g..16+4g+3}: vt_key_pos
#pragma unroll
                for (int qs = 0; qs < QS; ++qs) o[qs][dt] = mfma16(vf, pb[qs][kh], o[qs][dt]);
                if constexpr (SPLIT) {
                    const u32x4 vl = ld16(v_lds + VB_ + swz_v(row, kh * 4 + g));
#pragma unroll
                    for (int qs = 0; qs < QS; ++qs) {
                        o[qs][dt] = mfma16(vf, pbl[qs][kh], o[qs][dt]);
                        o[qs][dt] = mfma16(vl, pb[qs][kh], o[qs][dt]);
                    }
                }
            }
    }
    // ---- normalise and store: lane holds out[query j][d = dt*16 + g*4 .. +4]
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) {
        float l = l_run[qs];
        l += shfl_xor(l, 16);
        l += shfl_xor(l, 32);
        const float inv = 1.0f / l;
        const int query = q0 + wave * (QS * 16) + qs * 16 + j;
        if (query < p.T) {
            const size_t ldo = SPLIT ? (size_t)p.ldo : (size_t)p.H * HD;
            bf16_t* dst = p.out + ((size_t)b * p.T + query) * ldo + h * HD + g * 4;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const f32x4 v = o[qs][dt] * inv;
                const u32x2 hi = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
                st8(dst + dt * 16, hi);
                if constexpr (SPLIT)
                    st8(dst + p.lo_off + dt * 16, u32x2{pack_bf2(v[0] - bf2f_lo(hi[0]), v[1] - bf2f_hi(hi[0])),
                                                        pack_bf2(v[2] - bf2f_lo(hi[1]), v[3] - bf2f_hi(hi[1]))});
            }
        }
    }
}

// workgroup order (AttnArgs::sched, see attention_kernel): 0 = plain 3-D grid, 1 = XCD-grouped heads + heaviest query block first,
// 2 = heaviest first only, 3 = XCD-grouped only
static dim3 attention_grid(AttnArgs& a, int QB) {
    // measured (profiles/r03_l_*): causal prefill shape 2 < 3 < 0 = 1 (165-175 / 179-187 / 186-200 us); ViT shape 3 < 0 < 2
    // (78-85 / 85-92 / 88-94 us) — 2 for a causal pass, 3 otherwise
    a.nqb = (a.T + QB - 1) / QB;
    a.sched = a.causal ? 2 : 3;
    if ((a.sched == 1 || a.sched == 3) && (a.B * a.H) % 8 != 0) a.sched = a.sched == 1 ? 2 : 0;
    return a.sched ? dim3(a.nqb * a.H * a.B) : dim3(a.nqb, a.H, a.B);
}

// 8 waves x 16 queries keeps the hd-128 kernel at 128 VGPRs (two workgroups per CU)
template <int HD>
static void launch_attention_v(const AttnArgs& a0, hipStream_t s) {
    AttnArgs a = a0;
    const dim3 grid = attention_grid(a, 128), block(512);
#ifdef VC_EMU
    constexpr size_t shmem = 2 * (64 * HD * 2 + HD * 128);   // the two stages the product build holds in static LDS
#else
    constexpr size_t shmem = 0;
#endif
    if (a.causal) VC_LAUNCH((attention_kernel<HD, true, 8, 1>), grid, block, shmem, s, a);
    else VC_LAUNCH((attention_kernel<HD, false, 8, 1>), grid, block, shmem, s, a);
}

template <int HD>
static void launch_attention_split(const AttnArgs& a0, hipStream_t s) {
    AttnArgs a = a0;
    const dim3 grid = attention_grid(a, 128), block(512);
    constexpr size_t shmem = 2 * 2 * (64 * HD * 2 + HD * 128);   // [2 stages][K hi | K lo | V^T hi | V^T lo]
#ifndef VC_EMU
    static bool once = false;
    if (!once) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_kernel<HD, true, 8, 1, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_kernel<HD, false, 8, 1, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        once = true;
    }
#endif
    if (a.causal) VC_LAUNCH((attention_kernel<HD, true, 8, 1, true>), grid, block, shmem, s, a);
    else VC_LAUNCH((attention_kernel<HD, false, 8, 1, true>), grid, block, shmem, s, a);
}

void launch_attention(const AttnArgs& a, hipStream_t s) {
    if (a.q_lo != nullptr) {  // precision mode "split": hi / lo operand planes
        if (a.hd == 128) launch_attention_split<128>(a, s);
        else launch_attention_split<64>(a, s);
        return;
    }
    if (a.hd == 128) launch_attention_v<128>(a, s);
    else launch_attention_v<64>(a, s);
}

// =============================================================================================
// extend attention: n new queries of one (b,h) at positions P + t over the P + n keys of the DECODE cache (key-major K and V,
// bf16 or e4m3).  Workgroup = 64 queries as 4 waves x 16; key tiles of 64; MFMA 16x16x32 and the fp32 online softmax of
// attention_kernel (S^T = K Q^T, O^T = V^T P^T, the same fragment layouts and LDS swizzles).
//
// V arrives key-major, but O^T = V^T P^T wants V^T tiles.  The flash kernel's prefill gets them from a V^T scratch written by
// qkv_split; here the cache IS the operand, so the transpose happens in the register-staged LDS write: each thread loads 4 dims
// of the eight keys that make up one 16-byte chunk of the V^T key order (keys 4c..4c+3 and 16+4c..16+4c+3 of a 32-key block,
// vt_chunk_key0) and writes, per dim, that whole chunk — the transpose costs 4 ds_write_b128 per thread and tile, and no two
// threads share a 16-byte chunk.  Chosen over ds_read_b64_tr_b16 because (i) the e4m3 cache must pass through registers anyway to be
// widened, so one staging path serves both cache formats; (ii) the read side stays the flash kernel's conflict-free
// ds_read_b128 of a key-ordered V^T tile; (iii) the staging registers double as the prefetch of the next tile (its loads are
// in flight during the MFMAs of the current one), the form the guide rates best for attention forward.
// Keys past P + n (the cache's unwritten tail) are staged as zeros: a masked score is 0 after exp, but 0 x NaN is not.
// =============================================================================================
template <int HD, bool KV8>
__global__ __launch_bounds__(256) void attention_extend_kernel(AttnExtendArgs p) {
    static_assert(HD == 128, "the extend kernel's staging map covers hd 128");
    constexpr int WAVES = 4, QB = WAVES * 16;   // 64 queries per workgroup
    constexpr int KS = HD / 32, DT = HD / 16, KCH = HD / 8;
    constexpr int KB_ = 64 * HD * 2;            // K tile [64 keys][HD] bf16, then V^T tile [HD][64 keys]
    constexpr int KLD = 64 * KCH / 256;         // K chunks per thread and tile (4)
    using Raw = typename std::conditional<KV8, u32x2, u32x4>::type;   // 8 elements as they sit in the cache
    using Raw4 = typename std::conditional<KV8, uint32_t, u32x2>::type;   // 4 elements
    VC_DYNAMIC_SMEM(char, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int q0 = blockIdx.x * QB, h = blockIdx.y, b = blockIdx.z;
    const int n = p.n, P = p.P, Tk = P + n;
    const size_t bh = (size_t)b * p.H + h;
    constexpr int ESZ = KV8 ? 1 : 2;
    const char* kbase = reinterpret_cast<const char*>(p.k) + bh * p.kv_stride * (size_t)(HD * ESZ);
    const char* vbase = reinterpret_cast<const char*>(p.v) + bh * p.kv_stride * (size_t)(HD * ESZ);
    const bf16_t* qbase = p.q + bh * p.q_stride * HD;
    const uint8_t* km = p.key_mask != nullptr ? p.key_mask + (size_t)b * p.mask_stride : nullptr;

    u32x4 qf[KS];
    {
        const int qrow = min(q0 + wave * 16 + j, n - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = ld16(qbase + (size_t)qrow * HD + ks * 32 + g * 8);
    }
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const float c2 = p.scale * 1.4426950408889634f;
    const int kv_end = min(Tk, P + q0 + QB);
    const int nkt = (kv_end + 63) / 64;

    // staging map.  K: chunk c = i * 256 + tid -> key row c / KCH, 16-byte slot c % KCH (16 threads read one 256-byte row).
    // V: thread = (V^T chunk vch = tid / 32 of the tile: block vch / 4, c = vch % 4; dims 4 vd .. 4 vd + 3, vd = tid % 32)
    static_assert(HD / 4 == 32, "V staging: 32 threads per key row");
    const int vch = tid / 32, vd = tid % 32;
    const int vkey0 = (vch / 4) * 32 + (vch % 4) * 4;   // key of V^T position 8 vch + e: vkey0 + (e & 3) + 16 (e >> 2)
    Raw kr[KLD];
    Raw4 vr[8];
    auto load_tile = [&](int kt) {
        const int k0 = kt * 64;
#pragma unroll
        for (int i = 0; i < KLD; ++i) {
            const int c = i * 256 + tid, row = c / KCH, slot = c % KCH;
            if (k0 + row < Tk) kr[i] = *reinterpret_cast<const Raw*>(kbase + ((size_t)(k0 + row) * HD + slot * 8) * ESZ);
            else kr[i] = Raw{};
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = k0 + vkey0 + (e & 3) + 16 * (e >> 2);
            if (key < Tk) vr[e] = *reinterpret_cast<const Raw4*>(vbase + ((size_t)key * HD + vd * 4) * ESZ);
            else vr[e] = Raw4{};
        }
    };
    auto widen = [](const Raw& x) -> u32x4 {
        if constexpr (KV8) {
            const u32x2 lo = fp8x4_to_bf16x4(x[0]), hi = fp8x4_to_bf16x4(x[1]);
            return u32x4{lo[0], lo[1], hi[0], hi[1]};
        } else {
            return x;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < KLD; ++i) {
            const int c = i * 256 + tid, row = c / KCH, slot = c % KCH;
            st16(lds + swz_k<HD>(row, slot), widen(kr[i]));
        }
        // V^T: chunk vch of row d holds the eight keys' elements of dim d in position order
        u32x2 w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (KV8) w[e] = fp8x4_to_bf16x4(vr[e]);
            else w[e] = vr[e];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t sh = (i & 1) * 16;
            uint32_t x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (w[e][i >> 1] >> sh) & 0xFFFFu;
            st16(lds + KB_ + swz_v(vd * 4 + i, vch),
                 u32x4{x[0] | (x[1] << 16), x[2] | (x[3] << 16), x[4] | (x[5] << 16), x[6] | (x[7] << 16)});
        }
    };

    const int w_first = q0 + wave * 16;   // smallest query of this wave
    if (nkt > 0) load_tile(0);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();   // every wave is done reading the previous tile
        store_tile();
        __syncthreads();
        if (kt + 1 < nkt) load_tile(kt + 1);   // in flight under this tile's MFMAs
        const int k0 = kt * 64;
        if (w_first >= n || k0 > P + w_first + 15) continue;   // no query of the wave, or every key in their future
        f32x4 sacc[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) sacc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) sacc[sub] = mfma16(ld16(lds + swz_k<HD>(sub * 16 + j, ks * 4 + g)), qf[ks], sacc[sub]);
        const int query = w_first + j;
        if (k0 + 63 > P + w_first || k0 + 64 > Tk || km != nullptr) {   // a tile with a hidden key (wave-uniform)
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + sub * 16 + g * 4 + r;
                    if (key >= Tk || key > P + query || (km != nullptr && km[key] == 0)) sacc[sub][r] = -INFINITY;
                }
        }
        float mx = vmax3(sacc[0][0], sacc[0][1], sacc[0][2]);
        mx = vmax3(mx, sacc[0][3], sacc[1][0]);
        mx = vmax3(mx, sacc[1][1], sacc[1][2]);
        mx = vmax3(mx, sacc[1][3], sacc[2][0]);
        mx = vmax3(mx, sacc[2][1], sacc[2][2]);
        mx = vmax3(mx, sacc[2][3], sacc[3][0]);
        mx = vmax3(mx, sacc[3][1], sacc[3][2]);
        mx = vmax2(mx, sacc[3][3]);
        mx = rows_max(mx);
        // deferred maximum as in attention_kernel (the reference point moves only when a score exceeds it by e^8); key 0 is
        // visible to every query (causal from P >= 0; the engine checks the key mask), so the point is finite from tile 0 on
        constexpr float DEFER = 11.5f;
        const bool grew = wave_any((mx - m_run) * c2 > DEFER);
        const float m_new = grew ? vmax2(m_run, mx) : m_run;
        const float alpha = grew ? fast_exp2((m_run - m_new) * c2) : 1.0f;
        m_run = m_new;
        const float mc = m_new * c2;
        float rs = 0.f;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = fast_exp2(fmaf(sacc[sub][r], c2, -mc));   // hidden: 0
                sacc[sub][r] = e;
                rs += e;
            }
        if (grew) {
            l_run = l_run * alpha;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = o[dt] * alpha;
        }
        l_run += rs;
        u32x4 pb[2];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
            pb[kh] = u32x4{pack_bf2(sacc[2 * kh][0], sacc[2 * kh][1]), pack_bf2(sacc[2 * kh][2], sacc[2 * kh][3]),
                           pack_bf2(sacc[2 * kh + 1][0], sacc[2 * kh + 1][1]), pack_bf2(sacc[2 * kh + 1][2], sacc[2 * kh + 1][3])};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) o[dt] = mfma16(ld16(lds + KB_ + swz_v(dt * 16 + j, kh * 4 + g)), pb[kh], o[dt]);
    }
    float l = l_run;
    l += shfl_xor(l, 16);
    l += shfl_xor(l, 32);
    const int query = q0 + wave * 16 + j;
    if (query < n) {
        const float inv = 1.0f / l;
        bf16_t* dst = p.out + ((size_t)b * n + query) * ((size_t)p.H * HD) + h * HD + g * 4;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const f32x4 v = o[dt] * inv;
            st8(dst + dt * 16, u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])});
        }
    }
}

void launch_attention_extend(const AttnExtendArgs& a, hipStream_t s) {
    if (a.hd != 128) throw std::runtime_error("attention_extend: head dim 128 only");
    if (a.n < 1 || a.P < 0 || a.P + a.n > a.kv_stride) throw std::runtime_error("attention_extend: positions exceed the cache");
    const dim3 grid((a.n + 63) / 64, a.H, a.B), block(256);
    constexpr size_t shmem = 2 * 64 * 128 * 2;   // K tile + V^T tile
    if (a.kv8) VC_LAUNCH((attention_extend_kernel<128, true>), grid, block, shmem, s, a);
    else VC_LAUNCH((attention_extend_kernel<128, false>), grid, block, shmem, s, a);
}

// =============================================================================================
// fused decode attention: RoPE + KV append + softmax(q K^T) V for the one new token of each (b,h).
// One 512-thread workgroup per (b,h).  The cache holds K AND V key-major ([S][hd] per (b,h)), so both passes read one
// contiguous stream of 2 * hd bytes per key — 16 lanes per key row, 4 rows per wave-instruction, 8 independent
// non-temporal loads in flight per lane — and the append is two contiguous 2*hd-byte rows.  (Round 1 kept V transposed
// for the prefill's MFMA flash kernel and streamed hd strided rows of ctx*2 bytes here: 5.1-5.3 TB/s; the prefill now
// gets its V^T tiles from a per-call scratch and the cache layout serves the decode steps, which read it 127 times.)
//   phase 0  rotate q / k of the new token, append the K and V rows, q to LDS
//   phase 1  scores -> LDS (<= DEC_MAX_CTX keys)          [K stream]
//   phase 2  block softmax in LDS (the first V batch is already in flight)
//   phase 3  out = sum_key p[key] * V[key]                  [V stream]; lanes reduce over their 4 key rows, waves over LDS
// Row b takes its position from pos_dev[b * pos_stride]; rows with active_dev == 0 are skipped (the decode pool).
// =============================================================================================
constexpr int DEC_MAX_CTX = 4096;

// KV32 (precision mode "split"): the projection output and the K / V cache are fp32 (4 dims per 16-byte load, HD / 4 lanes
// per key row), q is not rounded, and the output row is written as bf16 hi / lo rows of a stacked group layout (out_G)
// KVF == 2: fp24 caches (rows of hd x u16 | hd x u8; 8 elements per lane = one 16-byte + one 8-byte load) — 3 bytes per element
// at 2^-17 relative precision: the split step's attention streams 0.75 of the fp32 bytes
// KVF == 3: e4m3 caches (rows of hd bytes) under the bf16 step — the fp8 weight format's KV: half the bf16 bytes
template <int HD, int UK, int KVF = 0>               // UK = independent row loads in flight per lane; KVF: 0 bf16, 1 fp32, 2 fp24, 3 e4m3
__global__ __launch_bounds__(512) void attention_decode_fused_kernel(AttnDecodeFusedArgs p) {
    constexpr bool KV32 = KVF == 1 || KVF == 2;   // the split step's operand forms (fp32 projection rows, unrounded q, hi / lo output rows)
    constexpr bool F24 = KVF == 2;
    constexpr bool F8 = KVF == 3;         // e4m3 caches under the bf16 step (the fp8 weight format): 16 elements per 16-byte load
    constexpr int EPL = KVF == 1 ? 4 : (F8 ? 16 : 8);   // elements per lane
    constexpr int ESZ = KVF == 1 ? 4 : (F8 ? 1 : 2);    // bytes per element of the (hi) plane
    constexpr int ROWB = F24 ? 3 * HD : HD * ESZ;   // bytes per cache row
    constexpr int LPK = HD / EPL;         // lanes per key row
    constexpr int KPW = 64 / LPK;         // key rows per wave-instruction
    constexpr int BATCH = 8 * KPW * UK;   // keys one round of the 8 waves covers
    __shared__ __attribute__((aligned(16))) float sc[DEC_MAX_CTX + BATCH];  // scores, padded to whole rounds
    __shared__ __attribute__((aligned(16))) float q_s[HD];
    __shared__ __attribute__((aligned(16))) float part[8][HD];
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    const size_t bh = (size_t)b * p.H + h;
    if (p.active_dev != nullptr && p.active_dev[(size_t)b * p.pos_stride] == 0) return;  // a free row of the decode pool
    stamp_begin(p.stamp, blockIdx.y * gridDim.x + blockIdx.x);
    const int pos = p.pos_dev[(size_t)b * p.pos_stride];
    const int ctx = pos + 1;
    const int D = p.H * HD;
    char* kbase = reinterpret_cast<char*>(p.k) + bh * p.kv_stride * ROWB;
    char* vbase = reinterpret_cast<char*>(p.v) + bh * p.kv_stride * ROWB;
    // Both streams run as a ROLLING window of UK loads per lane (phase 1 / 3 below).  wave-uniform base + one 32-bit byte offset per
    // lane (the scalar-base addressing form: half the address VGPRs); rows past the context are clamped to the last valid row
    constexpr int EPL_ = EPL;
    const int krow = lane / LPK, kcol = (lane % LPK) * EPL_;
    auto row_off = [&](int key) { return (uint32_t)(min(key, ctx - 1) * ROWB) + (uint32_t)(kcol * ESZ); };
    // fp24: the lo plane of the row, 8 bytes per lane
    auto lo_off = [&](int key) { return (uint32_t)(min(key, ctx - 1) * ROWB) + (uint32_t)(2 * HD + kcol); };
    u32x4 kv[UK];
    u32x2 kl[F24 ? UK : 1];
    auto first_k = [&]() {
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            kv[u] = ld16_stream(kbase + row_off(wave * KPW * UK + u * KPW + krow));
            if constexpr (F24) kl[u] = ld8_stream(kbase + lo_off(wave * KPW * UK + u * KPW + krow));
        }
    };
    // The first K batch (keys < BATCH) does not depend on phase 0 unless it contains the new token's own row: it is requested BEHIND
    // phase 0's operand loads and BEFORE its arithmetic and stores (round 6) — loads return in order, so the rotation waits for its
    // operands only, and the barrier's drain of the appended rows overlaps the batch's flight instead of preceding it (one HBM
    // round trip less per launch).  Requested unconditionally (a branch around it makes the compiler count the operands' wait for
    // the path WITHOUT the batch, i.e. wait for half of it); a context shorter than one round requests it again behind the
    // barrier, the only case in which the first request can have read the new row before it was written.
    const bool early = pos >= BATCH;
    // ---- phase 0: rotate q,k of the new token, append k / v to the cache (global) and keep q in LDS
    if (tid < HD / 2) {
        const int d = tid;
        const float c = p.rope_cos[(size_t)pos * (HD / 2) + d], s = p.rope_sin[(size_t)pos * (HD / 2) + d];
        if constexpr (KV32) {
            const float* row = reinterpret_cast<const float*>(p.qkv) + (size_t)b * (3 * D) + h * HD;
            const float q0 = row[d], q1 = row[d + HD / 2];
            const float k0 = row[D + d], k1 = row[D + d + HD / 2];
            const float v0 = row[2 * D + d], v1 = row[2 * D + d + HD / 2];
            first_k();
            q_s[d] = q0 * c - q1 * s;
            q_s[d + HD / 2] = q1 * c + q0 * s;
            if constexpr (F24) {
                auto put = [&](char* rowp, int dd, float val) {
                    const uint32_t code = f32_to_f24(val);
                    reinterpret_cast<uint16_t*>(rowp)[dd] = (uint16_t)(code >> 8);
                    reinterpret_cast<uint8_t*>(rowp + 2 * HD)[dd] = (uint8_t)(code & 0xFFu);
                };
                char* ko = kbase + (size_t)pos * ROWB;
                put(ko, d, k0 * c - k1 * s);
                put(ko, d + HD / 2, k1 * c + k0 * s);
                char* vo = vbase + (size_t)pos * ROWB;
                put(vo, d, v0);
                put(vo, d + HD / 2, v1);
            } else {
                float* ko = reinterpret_cast<float*>(kbase) + (size_t)pos * HD;
                ko[d] = k0 * c - k1 * s;
                ko[d + HD / 2] = k1 * c + k0 * s;
                float* vo = reinterpret_cast<float*>(vbase) + (size_t)pos * HD;
                vo[d] = v0;
                vo[d + HD / 2] = v1;
            }
        } else {
            const bf16_t* row = p.qkv + (size_t)b * (3 * D) + h * HD;
            const bf16_t rq0 = row[d], rq1 = row[d + HD / 2], rk0 = row[D + d], rk1 = row[D + d + HD / 2];
            const bf16_t v0 = row[2 * D + d], v1 = row[2 * D + d + HD / 2];
            first_k();
            const float q0 = bf2f(rq0), q1 = bf2f(rq1);
            const float k0 = bf2f(rk0), k1 = bf2f(rk1);
            q_s[d] = bf2f(f2bf(q0 * c - q1 * s));            // q is rounded to bf16 exactly like the unfused path
            q_s[d + HD / 2] = bf2f(f2bf(q1 * c + q0 * s));
            if constexpr (F8) {   // e4m3 rows: the bf16 values the bf16 cache would hold, re-rounded (as the prefill's writer does)
                uint8_t* ko = reinterpret_cast<uint8_t*>(kbase) + (size_t)pos * HD;
                ko[d] = f2fp8(bf2f(f2bf(k0 * c - k1 * s)));
                ko[d + HD / 2] = f2fp8(bf2f(f2bf(k1 * c + k0 * s)));
                uint8_t* vo = reinterpret_cast<uint8_t*>(vbase) + (size_t)pos * HD;
                vo[d] = f2fp8(bf2f(v0));
                vo[d + HD / 2] = f2fp8(bf2f(v1));
            } else {
                bf16_t* ko = reinterpret_cast<bf16_t*>(kbase) + (size_t)pos * HD;
                ko[d] = f2bf(k0 * c - k1 * s);
                ko[d + HD / 2] = f2bf(k1 * c + k0 * s);
                bf16_t* vo = reinterpret_cast<bf16_t*>(vbase) + (size_t)pos * HD;
                vo[d] = v0;
                vo[d + HD / 2] = v1;
            }
        }
    } else {
        first_k();
    }
    __syncthreads();  // workgroup-scope release/acquire: the appended K / V rows are visible to this block
    // ---- phase 1: scores
    float qv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) qv[e] = q_s[(lane % LPK) * EPL + e];
    const int ctx_pad = (ctx + BATCH - 1) / BATCH * BATCH;
    // keys hidden by the attention_mask of the row's prefill (vc_decode_step loops that keep a caller's mask; nullptr: none).
    // The new token's own key (position pos) is always visible.
    const uint8_t* kmask = p.key_mask != nullptr ? p.key_mask + (size_t)b * p.mask_stride : nullptr;
    // (a register of the rolling window is re-requested for the next batch as soon as its row has been consumed: UK rows in flight
    // with UK registers, no second set; no branch around the loads)
    auto dot = [&](const u32x4& r, const u32x2& rl) {
        float s = 0.f;
        if constexpr (F24) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += qv[e] * f24_elem(r, rl, e);
        } else if constexpr (F8) {
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                const f32x4 f = fp8x4_to_f32x4(r[w4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) s += qv[4 * w4 + e] * f[e];
            }
        } else if constexpr (KV32) {
            const f32x4 f = __builtin_bit_cast(f32x4, r);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += qv[e] * f[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) s += qv[2 * e] * bf2f_lo(r[e]) + qv[2 * e + 1] * bf2f_hi(r[e]);
        }
        return s;
    };
    if (!early) first_k();
    for (int kb = wave * KPW * UK; kb < ctx_pad; kb += BATCH) {
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int key = kb + u * KPW + krow;
            float s = dot(kv[u], kl[F24 ? u : 0]);
            kv[u] = ld16_stream(kbase + row_off(key + BATCH));
            if constexpr (F24) kl[u] = ld8_stream(kbase + lo_off(key + BATCH));
            s = lanes_sum<LPK>(s);
            if ((lane % LPK) == 0) sc[key] = (key < ctx && (kmask == nullptr || kmask[min(key, ctx - 1)] != 0)) ? s * p.scale : -INFINITY;
        }
    }
    // the first V batch of every wave does not depend on the scores: request it now so HBM stays busy through the
    // LDS-only softmax below
    u32x4 vv[UK];
    u32x2 vl[F24 ? UK : 1];
#pragma unroll
    for (int u = 0; u < UK; ++u) {
        vv[u] = ld16_stream(vbase + row_off(wave * KPW * UK + u * KPW + krow));
        if constexpr (F24) vl[u] = ld8_stream(vbase + lo_off(wave * KPW * UK + u * KPW + krow));
    }
    __syncthreads();
    // ---- phase 2: softmax over sc[0..ctx_pad)
    float mx = -INFINITY;
    for (int i = tid; i < ctx_pad; i += 512) mx = fmaxf(mx, sc[i]);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < 8; ++w) mx = fmaxf(mx, red[w]);
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < ctx_pad; i += 512) {
        const float e = __expf(sc[i] - mx);  // masked keys: exp(-inf) = 0
        sc[i] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) sum += red[w];
    const float inv = 1.0f / sum;
    // ---- phase 3: out[d] = sum_key p[key] * V[key][d]; a lane accumulates its dims over the key rows it loads (keys
    // past the context carry p = 0 and re-read the last valid row)
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int kb = wave * KPW * UK; kb < ctx_pad; kb += BATCH) {
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int key = kb + u * KPW + krow;
            const float pk = sc[key];
            const u32x4 v = vv[u];
            const u32x2 vlo = vl[F24 ? u : 0];
            vv[u] = ld16_stream(vbase + row_off(key + BATCH));
            if constexpr (F24) {
                vl[u] = ld8_stream(vbase + lo_off(key + BATCH));
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += pk * f24_elem(v, vlo, e);
            } else if constexpr (F8) {
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {
                    const f32x4 f = fp8x4_to_f32x4(v[w4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * w4 + e] += pk * f[e];
                }
            } else if constexpr (KV32) {
                const f32x4 f = __builtin_bit_cast(f32x4, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += pk * f[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[2 * e] += pk * bf2f_lo(v[e]);
                    acc[2 * e + 1] += pk * bf2f_hi(v[e]);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        float a = acc[e];
#pragma unroll
        for (int mk = LPK; mk < 64; mk <<= 1) a += shfl_xor(a, mk);  // over the KPW key rows of the wave-instruction
        acc[e] = a;
    }
    if (lane < LPK) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) part[wave][lane * EPL + e] = acc[e];
    }
    __syncthreads();
    if (tid < HD) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) a += part[w][tid];
        a *= inv;
        if constexpr (KV32) {  // stacked hi / lo row groups of the split decode GEMV: row b -> group b / G, slot b % G
            const int G = p.out_G;
            const size_t orow = (size_t)(b / G) * 2 * G + b % G;
            const bf16_t hi = f2bf(a);
            p.out[orow * D + h * HD + tid] = hi;
            p.out[(orow + G) * D + h * HD + tid] = f2bf(a - bf2f(hi));
        } else {
            p.out[(size_t)b * D + h * HD + tid] = f2bf(a);
        }
    }
    stamp_end(p.stamp, blockIdx.y * gridDim.x + blockIdx.x);
}

void launch_attention_decode_fused(const AttnDecodeFusedArgs& a, hipStream_t s) {
    const dim3 grid(a.H, a.B), block(512);
    // 8 row loads in flight per lane (8 KiB per wave, two workgroups per CU): 12 and 16 measured slower at every row count
    // (profiles/r05_u_kbench_dattn_uk.txt: 32 rows 99.4 / 103.4 / 108.7 us) and their instantiations were removed in round 5
    if (a.kv32 == 3) {  // bf16 step over e4m3 caches (the fp8 weight format)
        // rows in flight per lane: 16 elements per load cost 16 + 16 query / accumulator registers; 8 rows took 156 VGPRs (one
        // workgroup per CU); 6 rows: 124 VGPRs, two workgroups per CU (profiles/r04_n_kbench_dattn_kv8_uk.txt)
        if (a.hd == 128) {
            VC_LAUNCH((attention_decode_fused_kernel<128, 6, 3>), grid, block, 0, s, a);
        } else {
            VC_LAUNCH((attention_decode_fused_kernel<64, 4, 3>), grid, block, 0, s, a);
        }
        return;
    }
    if (a.kv32 == 2) {  // precision mode "split", fp24 caches
        // 6 rows x 24 B in flight per lane (the bf16 kernel's 8 x 16 B take 114 VGPRs, 8 rows of fp24 171: one workgroup per CU)
        if (a.hd == 128) VC_LAUNCH((attention_decode_fused_kernel<128, 6, 2>), grid, block, 0, s, a);
        else VC_LAUNCH((attention_decode_fused_kernel<64, 6, 2>), grid, block, 0, s, a);
        return;
    }
    if (a.kv32) {  // precision mode "split", fp32 caches
        if (a.hd == 128) VC_LAUNCH((attention_decode_fused_kernel<128, 8, 1>), grid, block, 0, s, a);
        else VC_LAUNCH((attention_decode_fused_kernel<64, 8, 1>), grid, block, 0, s, a);
        return;
    }
    if (a.hd == 128) {
        VC_LAUNCH((attention_decode_fused_kernel<128, 8>), grid, block, 0, s, a);
    } else {
        VC_LAUNCH((attention_decode_fused_kernel<64, 8>), grid, block, 0, s, a);
    }
}

// =============================================================================================
// Verify attention (speculative decoding): nq <= Q <= 8 consecutive query rows of ONE sequence — activation rows b * Q + j at
// positions pos + j — in one launch over one read of the K and the V stream.  Query j's output row and the cache rows appended for
// it are the bits attention_decode_fused_kernel gives that row in a step of its own, because per query nothing about the arithmetic
// changes: the key -> (wave, window slot, key row) map (UK, KPW and BATCH are the decode kernel's), lanes_sum over a key row's lanes,
// the per-thread stride-512 max / sum of the softmax followed by the wave and the 8-wave reductions, the lane and wave order of the V
// pass, __expf, the bf16 rounding of q.  What differs is invisible to a query: its score row runs to the CHUNK's padded end, and the
// keys between its own context and that end carry -inf -> p = 0 (they add +-0 to sums; an exactly-zero output may differ in sign),
// while the decode kernel re-reads its last valid row there, also under p = 0.
//   phase 0  64 threads per query: rotate q / k, append the K and V rows, q (bf16-rounded) to LDS
//   phase 1  every loaded key row dotted against the nq queries -> sc[j][key]; query j sees keys <= pos + j
//   phase 2  softmax per query
//   phase 3  V rows into nq accumulator sets; `part` serves the queries one after another
// Scores: Q rows of kv_stride + BATCH floats of dynamic LDS.
// =============================================================================================
// One accumulation acc + pk * v of the V pass, rounded as the COMPILED decode kernel rounds it.  The source of both kernels says
// `acc[e] += pk * v`; under the default contraction the back end makes that an fma for every element of a lane except its last
// two, whose accumulators the vectorizer turns into a two-wide add chain behind two-wide products (v_pk_mul_f32 + v_pk_add_f32 in
// every instantiation and both operand formats of attention_decode_fused_kernel): there the product is rounded before the add.
// In this kernel's larger loop body the same source line contracts everywhere, so the choice is spelled out here.  (The emulator
// build compiles both kernels for the host, where the plain expression means the same thing in both.)
template <bool LAST_PAIR> VC_DEV float vacc(float acc, float pk, float v) {
#ifdef VC_EMU
    return acc + pk * v;
#else
    if constexpr (LAST_PAIR) {
#pragma clang fp contract(off)
        const float t = pk * v;
        return acc + t;
    } else {
        return __builtin_fmaf(pk, v, acc);
    }
#endif
}

template <int HD, int UK, bool F8, int QM>
__global__ __launch_bounds__(512) void attention_verify_kernel(AttnVerifyArgs p) {
    constexpr int EPL = F8 ? 16 : 8;
    constexpr int ESZ = F8 ? 1 : 2;
    constexpr int ROWB = HD * ESZ;
    constexpr int LPK = HD / EPL;
    constexpr int KPW = 64 / LPK;
    constexpr int BATCH = 8 * KPW * UK;
    VC_DYNAMIC_SMEM(float, sc);   // [Q][kv_stride + BATCH]
    __shared__ __attribute__((aligned(16))) float q_s[QM][HD];
    __shared__ __attribute__((aligned(16))) float part[8][HD];
    __shared__ float red[QM][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    const size_t bh = (size_t)b * p.H + h;
    const int pos = p.pos_dev[(size_t)b * p.pos_stride];
    // queries of this sequence: none skips it; never more than the launch's Q or than the cache holds behind pos
    const int nq = min(min(p.nq_dev[b], min(p.Q, QM)), p.kv_stride - pos);
    if (nq <= 0 || pos < 0) return;
    const int srow = p.kv_stride + BATCH;
    const int ctx = pos + nq;   // keys of the last query
    const int D = p.H * HD;
    char* kbase = reinterpret_cast<char*>(p.k) + bh * p.kv_stride * ROWB;
    char* vbase = reinterpret_cast<char*>(p.v) + bh * p.kv_stride * ROWB;
    const int krow = lane / LPK, kcol = (lane % LPK) * EPL;
    auto row_off = [&](int key) { return (uint32_t)(min(key, ctx - 1) * ROWB) + (uint32_t)(kcol * ESZ); };
    // ---- phase 0: query j = tid / 64 at position pos + j
    {
        const int j = tid >> 6, d = tid & 63;
        if (j < nq && d < HD / 2) {
            const int pj = pos + j;
            const float c = p.rope_cos[(size_t)pj * (HD / 2) + d], s = p.rope_sin[(size_t)pj * (HD / 2) + d];
            const bf16_t* row = p.qkv + ((size_t)b * p.Q + j) * (3 * D) + h * HD;
            const bf16_t rq0 = row[d], rq1 = row[d + HD / 2], rk0 = row[D + d], rk1 = row[D + d + HD / 2];
            const bf16_t v0 = row[2 * D + d], v1 = row[2 * D + d + HD / 2];
            const float q0 = bf2f(rq0), q1 = bf2f(rq1);
            const float k0 = bf2f(rk0), k1 = bf2f(rk1);
            q_s[j][d] = bf2f(f2bf(q0 * c - q1 * s));
            q_s[j][d + HD / 2] = bf2f(f2bf(q1 * c + q0 * s));
            if constexpr (F8) {
                uint8_t* ko = reinterpret_cast<uint8_t*>(kbase) + (size_t)pj * HD;
                ko[d] = f2fp8(bf2f(f2bf(k0 * c - k1 * s)));
                ko[d + HD / 2] = f2fp8(bf2f(f2bf(k1 * c + k0 * s)));
                uint8_t* vo = reinterpret_cast<uint8_t*>(vbase) + (size_t)pj * HD;
                vo[d] = f2fp8(bf2f(v0));
                vo[d + HD / 2] = f2fp8(bf2f(v1));
            } else {
                bf16_t* ko = reinterpret_cast<bf16_t*>(kbase) + (size_t)pj * HD;
                ko[d] = f2bf(k0 * c - k1 * s);
                ko[d + HD / 2] = f2bf(k1 * c + k0 * s);
                bf16_t* vo = reinterpret_cast<bf16_t*>(vbase) + (size_t)pj * HD;
                vo[d] = v0;
                vo[d + HD / 2] = v1;
            }
        }
    }
    __syncthreads();  // workgroup-scope release/acquire: the appended K / V rows are visible to this block
    // ---- phase 1: scores of every query over one pass of the K stream
    const int ctx_pad = (ctx + BATCH - 1) / BATCH * BATCH;
    const uint8_t* kmask = p.key_mask != nullptr ? p.key_mask + (size_t)b * p.mask_stride : nullptr;
    u32x4 kv[UK];
    {
        // 8 queries of 16 elements would take 128 registers beside the rolling window: they are held as operand-format pairs (q is
        // rounded to that format, so the pair is exact) and widened at use
        constexpr bool PACKQ = F8 && QM == 8;
        float qv[PACKQ ? 1 : QM][EPL];
        uint32_t qp[PACKQ ? QM : 1][EPL / 2];
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            const float* qj = q_s[j < nq ? j : 0] + (lane % LPK) * EPL;
            if constexpr (PACKQ) {
#pragma unroll
                for (int e = 0; e < EPL / 2; ++e) qp[j][e] = pack_bf2(qj[2 * e], qj[2 * e + 1]);
            } else {
#pragma unroll
                for (int e = 0; e < EPL; ++e) qv[j][e] = qj[e];
            }
        }
        auto qe = [&](int j, int e) {
            if constexpr (PACKQ) return (e & 1) ? bf2f_hi(qp[j][e >> 1]) : bf2f_lo(qp[j][e >> 1]);
            else return qv[j][e];
        };
        auto dot = [&](const u32x4& r, int j) {
            float s = 0.f;
            if constexpr (F8) {
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {
                    const f32x4 f = fp8x4_to_f32x4(r[w4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s += qe(j, 4 * w4 + e) * f[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) s += qe(j, 2 * e) * bf2f_lo(r[e]) + qe(j, 2 * e + 1) * bf2f_hi(r[e]);
            }
            return s;
        };
#pragma unroll
        for (int u = 0; u < UK; ++u) kv[u] = ld16_stream(kbase + row_off(wave * KPW * UK + u * KPW + krow));
        for (int kb = wave * KPW * UK; kb < ctx_pad; kb += BATCH) {
#pragma unroll
            for (int u = 0; u < UK; ++u) {
                const int key = kb + u * KPW + krow;
                const u32x4 r = kv[u];
                kv[u] = ld16_stream(kbase + row_off(key + BATCH));
                const bool open = kmask == nullptr || kmask[min(key, ctx - 1)] != 0;
#pragma unroll
                for (int j = 0; j < QM; ++j) {
                    if (j < nq) {
                        float s = dot(r, j);
                        s = lanes_sum<LPK>(s);
                        if ((lane % LPK) == 0) sc[j * srow + key] = (key <= pos + j && open) ? s * p.scale : -INFINITY;
                    }
                }
            }
        }
    }
    u32x4 vv[UK];
#pragma unroll
    for (int u = 0; u < UK; ++u) vv[u] = ld16_stream(vbase + row_off(wave * KPW * UK + u * KPW + krow));
    __syncthreads();
    // ---- phase 2: softmax of every query over sc[j][0 .. ctx_pad)
    float inv[QM];
    {
        float mx[QM];
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            mx[j] = -INFINITY;
            if (j < nq) {
                for (int i = tid; i < ctx_pad; i += 512) mx[j] = fmaxf(mx[j], sc[j * srow + i]);
                mx[j] = wave_max(mx[j]);
                if (lane == 0) red[j][wave] = mx[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            if (j < nq) {
                mx[j] = red[j][0];
#pragma unroll
                for (int w = 1; w < 8; ++w) mx[j] = fmaxf(mx[j], red[j][w]);
            }
        }
        __syncthreads();
        float sum[QM];
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            sum[j] = 0.f;
            if (j < nq) {
                for (int i = tid; i < ctx_pad; i += 512) {
                    const float e = __expf(sc[j * srow + i] - mx[j]);
                    sc[j * srow + i] = e;
                    sum[j] += e;
                }
                sum[j] = wave_sum(sum[j]);
                if (lane == 0) red[j][wave] = sum[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            inv[j] = 0.f;
            if (j < nq) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) t += red[j][w];
                inv[j] = 1.0f / t;
            }
        }
    }
    // ---- phase 3: one pass of the V stream into nq accumulator sets
    float acc[QM][EPL];
#pragma unroll
    for (int j = 0; j < QM; ++j)
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[j][e] = 0.f;
    for (int kb = wave * KPW * UK; kb < ctx_pad; kb += BATCH) {
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int key = kb + u * KPW + krow;
            const u32x4 v = vv[u];
            vv[u] = ld16_stream(vbase + row_off(key + BATCH));
#pragma unroll
            for (int j = 0; j < QM; ++j) {
                if (j < nq) {
                    const float pk = sc[j * srow + key];
                    if constexpr (F8) {
#pragma unroll
                        for (int w4 = 0; w4 < 4; ++w4) {
                            const f32x4 f = fp8x4_to_f32x4(v[w4]);
                            acc[j][4 * w4] = vacc<false>(acc[j][4 * w4], pk, f[0]);
                            acc[j][4 * w4 + 1] = vacc<false>(acc[j][4 * w4 + 1], pk, f[1]);
                            if (w4 == 3) {
                                acc[j][14] = vacc<true>(acc[j][14], pk, f[2]);
                                acc[j][15] = vacc<true>(acc[j][15], pk, f[3]);
                            } else {
                                acc[j][4 * w4 + 2] = vacc<false>(acc[j][4 * w4 + 2], pk, f[2]);
                                acc[j][4 * w4 + 3] = vacc<false>(acc[j][4 * w4 + 3], pk, f[3]);
                            }
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 3; ++e) {
                            acc[j][2 * e] = vacc<false>(acc[j][2 * e], pk, bf2f_lo(v[e]));
                            acc[j][2 * e + 1] = vacc<false>(acc[j][2 * e + 1], pk, bf2f_hi(v[e]));
                        }
                        acc[j][6] = vacc<true>(acc[j][6], pk, bf2f_lo(v[3]));
                        acc[j][7] = vacc<true>(acc[j][7], pk, bf2f_hi(v[3]));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QM; ++j) {
        if (j < nq) {   // block-uniform: the barriers below are reached by every thread
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                float a = acc[j][e];
#pragma unroll
                for (int mk = LPK; mk < 64; mk <<= 1) a += shfl_xor(a, mk);
                acc[j][e] = a;
            }
            if (lane < LPK) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) part[wave][lane * EPL + e] = acc[j][e];
            }
            __syncthreads();
            if (tid < HD) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) a += part[w][tid];
                a *= inv[j];
                p.out[((size_t)b * p.Q + j) * D + h * HD + tid] = f2bf(a);
            }
            __syncthreads();   // `part` is free for the next query
        }
    }
}

template <int HD, int UK, bool F8, int QM>
static void launch_attention_verify_v(const AttnVerifyArgs& a, size_t lds, hipStream_t s) {
#ifndef VC_EMU
    static size_t allowed = 0;
    if (lds > 48 * 1024 && lds > allowed) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_verify_kernel<HD, UK, F8, QM>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        allowed = lds;
    }
#endif
    VC_LAUNCH((attention_verify_kernel<HD, UK, F8, QM>), dim3(a.H, a.B), dim3(512), lds, s, a);
}

// dynamic + static LDS of one workgroup of the verify attention; a launch needs it <= ATTN_VERIFY_LDS_MAX
size_t attention_verify_lds_bytes(int Q, int hd, int kv8, int kv_stride) {
    const int uk = kv8 ? (hd == 128 ? 6 : 4) : 8, epl = kv8 ? 16 : 8;
    const int batch = 8 * (64 / (hd / epl)) * uk;
    const int qm = Q <= 4 ? 4 : 8;
    return (size_t)Q * (kv_stride + batch) * 4 + (size_t)(qm + 8) * hd * 4 + (size_t)qm * 8 * 4;
}

void launch_attention_verify(const AttnVerifyArgs& a, hipStream_t s) {
    if (a.Q < 1 || a.Q > 8 || (a.hd != 128 && a.hd != 64)) throw std::runtime_error("attention_verify: Q in 1 .. 8, head dim 128 or 64");
    if (attention_verify_lds_bytes(a.Q, a.hd, a.kv8, a.kv_stride) > ATTN_VERIFY_LDS_MAX)
        throw std::runtime_error("attention_verify: the score rows of Q queries over this cache capacity exceed the LDS of a CU");
    const int uk = a.kv8 ? (a.hd == 128 ? 6 : 4) : 8, epl = a.kv8 ? 16 : 8;
    const size_t lds = (size_t)a.Q * (a.kv_stride + 8 * (64 / (a.hd / epl)) * uk) * 4;
    // the rows in flight per lane are the decode kernel's: they are part of the key -> lane map
    const bool q4 = a.Q <= 4;
    if (a.kv8) {
        if (a.hd == 128) q4 ? launch_attention_verify_v<128, 6, true, 4>(a, lds, s) : launch_attention_verify_v<128, 6, true, 8>(a, lds, s);
        else q4 ? launch_attention_verify_v<64, 4, true, 4>(a, lds, s) : launch_attention_verify_v<64, 4, true, 8>(a, lds, s);
    } else {
        if (a.hd == 128) q4 ? launch_attention_verify_v<128, 8, false, 4>(a, lds, s) : launch_attention_verify_v<128, 8, false, 8>(a, lds, s);
        else q4 ? launch_attention_verify_v<64, 8, false, 4>(a, lds, s) : launch_attention_verify_v<64, 8, false, 8>(a, lds, s);
    }
}

// =============================================================================================
// Fan-out attention (generate(num_return_sequences = n)): the n <= 8 rows g n .. g n + n - 1 of group g continue ONE prompt of P keys
// that sits in positions [0, P) of cache row `prefix_row[g]`; every row keeps its own keys P .. pos in ITS cache row.  All rows of a
// group stand at the same position pos >= P.  One workgroup per (group, head) is the verify kernel with a second, per-query stream
// behind the shared one: a prefix key row is loaded once and dotted against / accumulated into all n queries, a tail key row is
// loaded per query.  Row j's output and appended cache rows are the bits attention_decode_fused_kernel gives it over a cache row that
// holds prefix + own tail, for the verify kernel's reasons: key -> (wave, window slot, key row) is the decode kernel's map (UK, KPW,
// BATCH), lanes_sum, the stride-512 softmax reductions, the lane and wave order of the V pass, vacc.  A query's key sequence per
// lane is round by round, slot by slot, in both kernels; which of the two streams a round comes from does not enter the arithmetic.
// The split between the streams is per (wave, round): the KPW * UK keys a wave covers in one round are shared when all of them lie
// below P, else the round is loaded per query, each lane taking its key from the prefix row (key < P) or the query's own row.
// Keys behind pos, up to the padded end, carry -inf (the decode kernel's padded end is the same: one position for all queries).
//   phase 0  64 threads per query: rotate q / k at pos, append K and V to the row's OWN cache row, q (bf16-rounded) to LDS
//   phase 1  shared rounds: one load, n dots; tail rounds: per query — both as one rolling window of UK loads per lane
//   phase 2  softmax per query
//   phase 3  the V stream the same way into n accumulator sets; `part` serves the queries one after another
// Scores: n rows of kv_stride + BATCH floats of dynamic LDS.  No key mask (generate()'s cached steps run under an all-ones mask).
// =============================================================================================
template <int HD, int UK, bool F8, int QM>
__global__ __launch_bounds__(512) void attention_fanout_kernel(AttnFanoutArgs p) {
    constexpr int EPL = F8 ? 16 : 8;
    constexpr int ESZ = F8 ? 1 : 2;
    constexpr int ROWB = HD * ESZ;
    constexpr int LPK = HD / EPL;
    constexpr int KPW = 64 / LPK;
    constexpr int WR = KPW * UK;          // keys one wave covers per round
    constexpr int BATCH = 8 * WR;
    VC_DYNAMIC_SMEM(float, sc);   // [n][kv_stride + BATCH]
    __shared__ __attribute__((aligned(16))) float q_s[QM][HD];
    __shared__ __attribute__((aligned(16))) float part[8][HD];
    __shared__ float red[QM][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, g = blockIdx.y;
    const int nq = min(p.n, QM);
    const int r0 = g * p.n;                                   // first row of the group
    const int pos = p.pos_dev[(size_t)r0 * p.pos_stride];
    const int P = p.P_dev[g];
    const int prow = p.prefix_row_dev != nullptr ? p.prefix_row_dev[g] : g;
    // nothing is touched for a group whose description does not fit the cache
    if (nq <= 0 || P < 0 || pos < P || pos >= p.kv_stride || prow < 0 || prow >= p.cache_rows || r0 + nq > p.cache_rows) return;
    const int srow = p.kv_stride + BATCH;
    const int ctx = pos + 1;
    const int D = p.H * HD;
    const size_t head_bytes = (size_t)p.kv_stride * ROWB;
    const char* kpre = reinterpret_cast<const char*>(p.k) + ((size_t)prow * p.H + h) * head_bytes;
    const char* vpre = reinterpret_cast<const char*>(p.v) + ((size_t)prow * p.H + h) * head_bytes;
    char* kown0 = reinterpret_cast<char*>(p.k) + ((size_t)r0 * p.H + h) * head_bytes;   // query j's own (row, head): + j * own_step
    char* vown0 = reinterpret_cast<char*>(p.v) + ((size_t)r0 * p.H + h) * head_bytes;
    const size_t own_step = (size_t)p.H * head_bytes;
    const int krow = lane / LPK, kcol = (lane % LPK) * EPL;
    // a shared round reads the prefix row (keys < P; the window's look-ahead is clamped into it); a tail round takes key < P from the
    // prefix row and the others, clamped to pos, from the query's own row
    auto pre_off = [&](int key) { return (uint32_t)(min(key, P - 1) * ROWB) + (uint32_t)(kcol * ESZ); };
    auto tail_at = [&](const char* pre, const char* own, int key) {
        const int kk = min(key, pos);
        return (kk < P ? pre : own) + ((uint32_t)(kk * ROWB) + (uint32_t)(kcol * ESZ));
    };
    // ---- phase 0: query j = tid / 64, all at position pos
    {
        const int j = tid >> 6, d = tid & 63;
        if (j < nq && d < HD / 2) {
            const float c = p.rope_cos[(size_t)pos * (HD / 2) + d], s = p.rope_sin[(size_t)pos * (HD / 2) + d];
            const bf16_t* row = p.qkv + (size_t)(r0 + j) * (3 * D) + h * HD;
            const bf16_t rq0 = row[d], rq1 = row[d + HD / 2], rk0 = row[D + d], rk1 = row[D + d + HD / 2];
            const bf16_t v0 = row[2 * D + d], v1 = row[2 * D + d + HD / 2];
            const float q0 = bf2f(rq0), q1 = bf2f(rq1);
            const float k0 = bf2f(rk0), k1 = bf2f(rk1);
            q_s[j][d] = bf2f(f2bf(q0 * c - q1 * s));
            q_s[j][d + HD / 2] = bf2f(f2bf(q1 * c + q0 * s));
            char* kb_ = kown0 + j * own_step;
            char* vb_ = vown0 + j * own_step;
            if constexpr (F8) {
                uint8_t* ko = reinterpret_cast<uint8_t*>(kb_) + (size_t)pos * HD;
                ko[d] = f2fp8(bf2f(f2bf(k0 * c - k1 * s)));
                ko[d + HD / 2] = f2fp8(bf2f(f2bf(k1 * c + k0 * s)));
                uint8_t* vo = reinterpret_cast<uint8_t*>(vb_) + (size_t)pos * HD;
                vo[d] = f2fp8(bf2f(v0));
                vo[d + HD / 2] = f2fp8(bf2f(v1));
            } else {
                bf16_t* ko = reinterpret_cast<bf16_t*>(kb_) + (size_t)pos * HD;
                ko[d] = f2bf(k0 * c - k1 * s);
                ko[d + HD / 2] = f2bf(k1 * c + k0 * s);
                bf16_t* vo = reinterpret_cast<bf16_t*>(vb_) + (size_t)pos * HD;
                vo[d] = v0;
                vo[d + HD / 2] = v1;
            }
        }
    }
    __syncthreads();  // workgroup-scope release/acquire: the appended K / V rows are visible to this block
    const int ctx_pad = (ctx + BATCH - 1) / BATCH * BATCH;
    // this wave's rounds start at keys wave * WR + r * BATCH; the first n_sh of them lie below P as a whole
    const int kb0 = wave * WR;
    const int n_sh = P >= kb0 + WR ? (P - kb0 - WR) / BATCH + 1 : 0;
    const int kb_tail = kb0 + n_sh * BATCH;       // first tail round (>= ctx_pad: none)
    // ---- phase 1: scores
    u32x4 kv[UK];
    {
        constexpr bool PACKQ = F8 && QM == 8;   // as the verify kernel: 8 queries of 16 elements are held as operand-format pairs
        float qv[PACKQ ? 1 : QM][EPL];
        uint32_t qp[PACKQ ? QM : 1][EPL / 2];
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            const float* qj = q_s[j < nq ? j : 0] + (lane % LPK) * EPL;
            if constexpr (PACKQ) {
#pragma unroll
                for (int e = 0; e < EPL / 2; ++e) qp[j][e] = pack_bf2(qj[2 * e], qj[2 * e + 1]);
            } else {
#pragma unroll
                for (int e = 0; e < EPL; ++e) qv[j][e] = qj[e];
            }
        }
        auto qe = [&](int j, int e) {
            if constexpr (PACKQ) return (e & 1) ? bf2f_hi(qp[j][e >> 1]) : bf2f_lo(qp[j][e >> 1]);
            else return qv[j][e];
        };
        auto dot = [&](const u32x4& r, int j) {
            float s = 0.f;
            if constexpr (F8) {
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {
                    const f32x4 f = fp8x4_to_f32x4(r[w4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s += qe(j, 4 * w4 + e) * f[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) s += qe(j, 2 * e) * bf2f_lo(r[e]) + qe(j, 2 * e + 1) * bf2f_hi(r[e]);
            }
            return s;
        };
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int key = kb0 + u * KPW + krow;
            kv[u] = n_sh > 0 ? ld16_stream(kpre + pre_off(key)) : ld16_stream(tail_at(kpre, kown0, key));
        }
        for (int kb = kb0; kb < kb_tail; kb += BATCH) {
            const bool last = kb + BATCH >= kb_tail;     // the look-ahead of the last shared round: query 0's first tail round
#pragma unroll
            for (int u = 0; u < UK; ++u) {
                const int key = kb + u * KPW + krow;
                const u32x4 r = kv[u];
                kv[u] = last ? ld16_stream(tail_at(kpre, kown0, key + BATCH)) : ld16_stream(kpre + pre_off(key + BATCH));
#pragma unroll
                for (int j = 0; j < QM; ++j) {
                    if (j < nq) {
                        float s = dot(r, j);
                        s = lanes_sum<LPK>(s);
                        if ((lane % LPK) == 0) sc[j * srow + key] = s * p.scale;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            if (j < nq) {
                const char* own = kown0 + j * own_step;
                const char* nxt = kown0 + (j + 1 < nq ? j + 1 : j) * own_step;
                for (int kb = kb_tail; kb < ctx_pad; kb += BATCH) {
                    const bool last = kb + BATCH >= ctx_pad;   // look-ahead: the next query's first tail round
#pragma unroll
                    for (int u = 0; u < UK; ++u) {
                        const int key = kb + u * KPW + krow;
                        const u32x4 r = kv[u];
                        kv[u] = ld16_stream(last ? tail_at(kpre, nxt, kb_tail + u * KPW + krow) : tail_at(kpre, own, key + BATCH));
                        float s = dot(r, j);
                        s = lanes_sum<LPK>(s);
                        if ((lane % LPK) == 0) sc[j * srow + key] = key <= pos ? s * p.scale : -INFINITY;
                    }
                }
            }
        }
    }
    u32x4 vv[UK];
#pragma unroll
    for (int u = 0; u < UK; ++u) {
        const int key = kb0 + u * KPW + krow;
        vv[u] = n_sh > 0 ? ld16_stream(vpre + pre_off(key)) : ld16_stream(tail_at(vpre, vown0, key));
    }
    __syncthreads();
    // ---- phase 2: softmax of every query over sc[j][0 .. ctx_pad)
    float inv[QM];
    {
        float mx[QM];
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            mx[j] = -INFINITY;
            if (j < nq) {
                for (int i = tid; i < ctx_pad; i += 512) mx[j] = fmaxf(mx[j], sc[j * srow + i]);
                mx[j] = wave_max(mx[j]);
                if (lane == 0) red[j][wave] = mx[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            if (j < nq) {
                mx[j] = red[j][0];
#pragma unroll
                for (int w = 1; w < 8; ++w) mx[j] = fmaxf(mx[j], red[j][w]);
            }
        }
        __syncthreads();
        float sum[QM];
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            sum[j] = 0.f;
            if (j < nq) {
                for (int i = tid; i < ctx_pad; i += 512) {
                    const float e = __expf(sc[j * srow + i] - mx[j]);
                    sc[j * srow + i] = e;
                    sum[j] += e;
                }
                sum[j] = wave_sum(sum[j]);
                if (lane == 0) red[j][wave] = sum[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QM; ++j) {
            inv[j] = 0.f;
            if (j < nq) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) t += red[j][w];
                inv[j] = 1.0f / t;
            }
        }
    }
    // ---- phase 3: the V stream into nq accumulator sets
    float acc[QM][EPL];
#pragma unroll
    for (int j = 0; j < QM; ++j)
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[j][e] = 0.f;
    auto accum = [&](float* a, float pk, const u32x4& v) {   // the verify kernel's accumulation of one V row into one query's set
        if constexpr (F8) {
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                const f32x4 f = fp8x4_to_f32x4(v[w4]);
                a[4 * w4] = vacc<false>(a[4 * w4], pk, f[0]);
                a[4 * w4 + 1] = vacc<false>(a[4 * w4 + 1], pk, f[1]);
                if (w4 == 3) {
                    a[14] = vacc<true>(a[14], pk, f[2]);
                    a[15] = vacc<true>(a[15], pk, f[3]);
                } else {
                    a[4 * w4 + 2] = vacc<false>(a[4 * w4 + 2], pk, f[2]);
                    a[4 * w4 + 3] = vacc<false>(a[4 * w4 + 3], pk, f[3]);
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                a[2 * e] = vacc<false>(a[2 * e], pk, bf2f_lo(v[e]));
                a[2 * e + 1] = vacc<false>(a[2 * e + 1], pk, bf2f_hi(v[e]));
            }
            a[6] = vacc<true>(a[6], pk, bf2f_lo(v[3]));
            a[7] = vacc<true>(a[7], pk, bf2f_hi(v[3]));
        }
    };
    for (int kb = kb0; kb < kb_tail; kb += BATCH) {
        const bool last = kb + BATCH >= kb_tail;
#pragma unroll
        for (int u = 0; u < UK; ++u) {
            const int key = kb + u * KPW + krow;
            const u32x4 v = vv[u];
            vv[u] = last ? ld16_stream(tail_at(vpre, vown0, key + BATCH)) : ld16_stream(vpre + pre_off(key + BATCH));
#pragma unroll
            for (int j = 0; j < QM; ++j) {
                if (j < nq) accum(acc[j], sc[j * srow + key], v);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QM; ++j) {
        if (j < nq) {
            const char* own = vown0 + j * own_step;
            const char* nxt = vown0 + (j + 1 < nq ? j + 1 : j) * own_step;
            for (int kb = kb_tail; kb < ctx_pad; kb += BATCH) {
                const bool last = kb + BATCH >= ctx_pad;
#pragma unroll
                for (int u = 0; u < UK; ++u) {
                    const int key = kb + u * KPW + krow;
                    const u32x4 v = vv[u];
                    vv[u] = ld16_stream(last ? tail_at(vpre, nxt, kb_tail + u * KPW + krow) : tail_at(vpre, own, key + BATCH));
                    accum(acc[j], sc[j * srow + key], v);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QM; ++j) {
        if (j < nq) {   // block-uniform: the barriers below are reached by every thread
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                float a = acc[j][e];
#pragma unroll
                for (int mk = LPK; mk < 64; mk <<= 1) a += shfl_xor(a, mk);
                acc[j][e] = a;
            }
            if (lane < LPK) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) part[wave][lane * EPL + e] = acc[j][e];
            }
            __syncthreads();
            if (tid < HD) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) a += part[w][tid];
                a *= inv[j];
                p.out[(size_t)(r0 + j) * D + h * HD + tid] = f2bf(a);
            }
            __syncthreads();   // `part` is free for the next query
        }
    }
}

template <int HD, int UK, bool F8, int QM>
static void launch_attention_fanout_v(const AttnFanoutArgs& a, size_t lds, hipStream_t s) {
#ifndef VC_EMU
    static size_t allowed = 0;
    if (lds > 48 * 1024 && lds > allowed) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_fanout_kernel<HD, UK, F8, QM>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        allowed = lds;
    }
#endif
    VC_LAUNCH((attention_fanout_kernel<HD, UK, F8, QM>), dim3(a.H, a.G), dim3(512), lds, s, a);
}

// dynamic + static LDS of one workgroup of the fan-out attention; a launch needs it <= ATTN_VERIFY_LDS_MAX
size_t attention_fanout_lds_bytes(int n, int hd, int kv8, int kv_stride) { return attention_verify_lds_bytes(n, hd, kv8, kv_stride); }

void launch_attention_fanout(const AttnFanoutArgs& a, hipStream_t s) {
    if (a.n < 1 || a.n > 8 || (a.hd != 128 && a.hd != 64)) throw std::runtime_error("attention_fanout: n in 1 .. 8, head dim 128 or 64");
    if (attention_fanout_lds_bytes(a.n, a.hd, a.kv8, a.kv_stride) > ATTN_VERIFY_LDS_MAX)
        throw std::runtime_error("attention_fanout: the score rows of n queries over this cache capacity exceed the LDS of a CU");
    const int uk = a.kv8 ? (a.hd == 128 ? 6 : 4) : 8, epl = a.kv8 ? 16 : 8;
    const size_t lds = (size_t)a.n * (a.kv_stride + 8 * (64 / (a.hd / epl)) * uk) * 4;
    // the rows in flight per lane are the decode kernel's: they are part of the key -> lane map
    const bool q4 = a.n <= 4;
    if (a.kv8) {
        if (a.hd == 128) q4 ? launch_attention_fanout_v<128, 6, true, 4>(a, lds, s) : launch_attention_fanout_v<128, 6, true, 8>(a, lds, s);
        else q4 ? launch_attention_fanout_v<64, 4, true, 4>(a, lds, s) : launch_attention_fanout_v<64, 4, true, 8>(a, lds, s);
    } else {
        if (a.hd == 128) q4 ? launch_attention_fanout_v<128, 8, false, 4>(a, lds, s) : launch_attention_fanout_v<128, 8, false, 8>(a, lds, s);
        else q4 ? launch_attention_fanout_v<64, 8, false, 4>(a, lds, s) : launch_attention_fanout_v<64, 8, false, 8>(a, lds, s);
    }
}

}  // namespace vc
