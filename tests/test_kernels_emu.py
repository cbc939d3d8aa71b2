"""CPU tests of the HIP kernels' logic through the thread-per-lane emulator (tests/emu): index math,
LDS layouts/swizzles, MFMA fragment plumbing, reductions, masks — at small shapes, against the oracle.
These do NOT prove hardware semantics (that is what `-m gpu` is for); they keep the GPU budget for
measurement instead of debugging."""
import pytest

import kernel_cases as kc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


GEMM_CASES = [(128, 128, 64, 3, True), (200, 136, 128, 0, True), (70, 264, 192, 1, True), (64, 128, 64, 2, True),
              (100, 128, 128, 4, False), (100, 256, 64, 5, False)]
GEMM_F8_CASES = [(100, 144, 128, 0), (300, 272, 256, 4), (70, 528, 384, 5), (16, 16, 128, 0)]
QKV_CASES = [(2, 96, 2, 128, False, 0, False, False), (2, 70, 2, 192, True, 0, False, False), (3, 133, 4, 128, False, 0, False, True),
             (1, 64, 2, 256, False, 0, True, True)]


@pytest.fixture(scope="module")
def be16():
    """libvcoder_emu_f16.so: the same sources built with -DVC_F16 (IEEE fp16 MFMA operands)"""
    return kc.EmuBackend("fp16")


# (B, n, H, hd, P, kv8): qkv_split as a continuation calls it — n ragged, P off the 64-key grid
QKV_OFFSET_CASES = [(1, 21, 2, 128, 75, False), (2, 5, 2, 128, 130, True), (1, 70, 1, 64, 37, False), (3, 13, 2, 128, 1, True),
                    (1, 99, 2, 128, 89, True)]


@pytest.mark.parametrize("M,N,K,epi,bias", GEMM_CASES)
def test_gemm(be, M, N, K, epi, bias):
    kc.check_gemm(be, M, N, K, epi, bias, path=_path(be, "dma"))


def _path(be, default):
    """the kernel the launcher must choose for the small bf16 shapes of this file: the 128 x 128 one unless the test hook is on"""
    return "8phase" if getattr(be, "forced_8phase", False) else default


@pytest.mark.parametrize("M,N,K,epi,bias", GEMM_CASES)
def test_gemm_padded_rows(be, M, N, K, epi, bias):
    """the activation rows with the row stride of a prefill's RMSNorm output (lda = K + 64, NaN in the pad, the array ending behind
    the last row's valid columns), and the weight rows strided as well: same tolerance, same bits as lda = ldw = K"""
    kc.check_gemm(be, M, N, K, epi, bias, lda_pad=64, path=_path(be, "dma"))
    kc.check_gemm(be, M, N, K, epi, bias, seed=1, lda_pad=64, ldw_pad=8 * (1 + epi), ws_mb=1, path=_path(be, "dma"))   # through vck_gemm_ws


def test_gemm_splitk_remainder_round(be):
    """260 tiles of 256x256 = one full round + 4 remainder tiles, cut into 2 K-slices each and finished by the fix-up
    launch (bias + quick-GELU epilogue; ragged M); again over activation rows of stride K + 64, bit for bit."""
    kc.check_gemm(be, 1000 + 24, 16640 - 8, 128, 1, True, seed=2, ws_mb=4, lda_pad=64, path="8phase")


@pytest.mark.parametrize("M,N,K,epi", [(8, 64, 256, 0), (3, 32, 1024, 1), (16, 48, 288, 2), (8, 64, 256, 3),
                                       (1, 16, 32, 1)] + kc.GEMV_TABLE_CASES)
def test_gemv(be, M, N, K, epi):
    kc.check_gemv(be, M, N, K, epi)


@pytest.mark.parametrize("M,N,K,epi,norm", [(8, 64, 256, 0, False), (3, 32, 1024, 1, False), (16, 48, 320, 2, False),
                                            (8, 64, 256, 3, False), (1, 16, 64, 1, False), (8, 64, 512, 0, True),
                                            (16, 32, 5120, 3, True), (5, 32, 320, 1, True)] + kc.GEMV_FP8_TABLE_CASES)
def test_gemv_fp8(be, M, N, K, epi, norm):
    kc.check_gemv_fp8(be, M, N, K, epi, norm)


@pytest.mark.parametrize("M,N,K,epi", GEMM_F8_CASES)
def test_gemm_f8(be, M, N, K, epi):
    kc.check_gemm_f8(be, M, N, K, epi, path="8phase")


def test_gemm_f8_splitk_remainder_round(be):
    """one full round of 256 tiles + 4 remainder tiles cut into K-slices; scales applied by the fix-up launch"""
    kc.check_gemm_f8(be, 1000 + 24, 16640 - 16, 256, 0, seed=3, ws_mb=4)


@pytest.mark.parametrize("M,N,K,ks", [(8, 64, 512, 2), (16, 48, 320, 3), (3, 32, 1024, 4), (8, 32, 64, 4)])
def test_gemv_splitk(be, M, N, K, ks):
    kc.check_gemv_splitk(be, M, N, K, ks)


@pytest.mark.parametrize("N,K,epi,norm,ks", [(32, 256, 0, True, 0), (48, 320, 1, True, 0), (64, 256, 3, True, 0),
                                              (32, 512, 2, False, 0), (48, 320, 1, False, 3), (32, 1024, 0, True, 2)])
def test_gemv_32_rows(be, N, K, epi, norm, ks):
    """M in 17..32 (the decode pool): two row groups per weight pass, bit-identical per row to the 16-row pass."""
    kc.check_gemv_rows_agree_across_variants(be, N, K, epi, norm, ks)


@pytest.mark.parametrize("N,K,epi,norm", [(24576, 128, 3, True), (64, 256, 0, True), (4096, 192, 2, False),
                                          (16 * 767, 128, 0, True), (16 * 900, 192, 0, False), (16 * 1376, 128, 3, True), (16 * 1727, 64, 3, True)])
def test_gemv_32_rows_w8a16(be, N, K, epi, norm):
    """the same promise with e4m3 weights; the matrices of more than 512 tiles take the one-workgroup-per-CU geometry at 17..32 rows
    since round 6 (3 / 4 / 6 / 7 tiles per workgroup, ragged last workgroup included), whose finishing stage gives every wave
    several (tile, row group) units — against the pair geometry that serves the same rows in 8- and 16-row passes"""
    kc.check_gemv_rows_agree_across_variants(be, N, K, epi, norm, fp8=True)


@pytest.mark.parametrize("N,K,epi,norm,ks,fp8,M,buffers", kc.GEMV_SPLITK_TABLE_CASES)
def test_gemv_splitk_geometries_17_to_32_rows(be, N, K, epi, norm, ks, fp8, M, buffers):
    """the split-K cells of the geometry table at 17..24 and 25..32 rows (and the <= 8- / <= 16-row cells of their sub-passes), bf16
    and W8A16: the same bits per row from every pass, within the float64 bar"""
    kc.check_gemv_rows_agree_across_variants(be, N, K, epi, norm, ks, fp8=fp8, M=M, buffers=buffers)


def test_gemv_chain_24_rows(be):
    kc.check_gemv_norm_chain(be, 24, 256, 64, seed=7)
    kc.check_gemv_norm_chain(be, 32, 512, 96, seed=8)


def test_interleave(be):
    kc.check_interleave(be, 24, 64)


@pytest.mark.parametrize("rows,D", [(5, 128), (9, 1024)])
def test_layernorm(be, rows, D):
    kc.check_layernorm(be, rows, D)


@pytest.mark.parametrize("rows,D,gather", [(3, 256, False), (6, 4096, False), (2, 5120, True), (9, 5120, False)])
def test_rmsnorm(be, rows, D, gather):
    kc.check_rmsnorm(be, rows, D, gather)


@pytest.mark.parametrize("rows,D", [(9, 256), (5, 1280), (3, 5120)])
def test_rmsnorm_q8(be, rows, D):
    kc.check_rmsnorm_q8(be, rows, D)
    kc.check_quant_act_rows_exhaustive(be)


def test_vit_front(be):
    kc.check_im2col(be, 2, 56, 14, 640)
    kc.check_vit_embed_ln(be, 2, 17, 128)
    kc.check_select_rows(be, 2, 17, 128)


@pytest.mark.parametrize("B,T,H,hd,rope", [(1, 70, 2, 128, True), (2, 17, 2, 64, False)])
def test_qkv_split(be, B, T, H, hd, rope):
    kc.check_qkv_split(be, B, T, H, hd, rope)


@pytest.mark.parametrize("B,n,H,hd,P,kv8", QKV_OFFSET_CASES)
def test_qkv_split_at_offset(be, B, n, H, hd, P, kv8):
    kc.check_qkv_split_at_offset(be, B, n, H, hd, P, kv8)



@pytest.mark.parametrize("B,H,T,hd,causal,spike", [(1, 1, 17, 64, False, False), (1, 2, 150, 64, False, True),
                                                   (1, 1, 70, 128, True, False), (1, 1, 200, 128, True, True),
                                                   (2, 4, 300, 128, True, True), (4, 2, 150, 64, False, False)])  # B H % 8 == 0: XCD-grouped order
def test_attention(be, B, H, T, hd, causal, spike):
    kc.check_attention(be, B, H, T, hd, causal, spike=spike)


# ---- the attention kernels as the engine calls them: key masks, the prefill's strides, poison behind every limit, causal needles -------
# (B, H, T, hd, causal, mask pattern per batch row, needle)
ATTN_EX_CASES = [(3, 1, 330, 128, True, ["pad200", "early", "ones"], True), (2, 2, 200, 128, True, ["straddle", "pad63"], True),
                 (4, 2, 150, 64, True, ["tile", "pad64", "singles", "pad1"], True),      # B H % 8 == 0: XCD-grouped order
                 (2, 1, 70, 64, False, ["pad1", "singles"], False), (1, 2, 257, 128, False, ["straddle"], False),
                 (1, 1, 192, 128, True, None, True), (1, 2, 129, 128, True, None, False),
                 (2, 2, 150, 64, False, None, False)]    # no mask, non-causal, T off the 64 grid: key T sits inside the last tile


@pytest.mark.parametrize("B,H,T,hd,causal,patterns,needle", ATTN_EX_CASES)
def test_attention_ex(be, B, H, T, hd, causal, patterns, needle):
    """vck_attention_ex: q_stride = T, kv_stride = T + 128, vt_stride = T rounded to 64, mask stride 4096"""
    kc.check_attention_ex(be, B, H, T, hd, causal, patterns, needle, seed=T)


def test_attention_ex_fp16_operand_library(be16):
    kc.check_attention_ex(be16, 3, 1, 330, 128, True, ["pad200", "early", "ones"], True, seed=1)
    kc.check_attention_ex(be16, 2, 2, 150, 64, False, ["tile", "pad1"], False, seed=2)
    kc.check_attention(be16, 1, 2, 200, 128, True, spike=True)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_attention_decode_masked(be, fmt):
    """the fused decode attention in its four cache formats with a position and a key mask per row, one row inactive"""
    kc.check_attention_decode_masked(be, fmt, 5, 2, 128, 329, ["pad200", "early", "straddle", "ones", "pad1"], seed=fmt)
    kc.check_attention_decode_masked(be, fmt, 4, 1, 64, 140, ["tile", "singles", "pad63", "pad64"], seed=10 + fmt)
    kc.check_attention_decode_masked(be, fmt, 1, 1, 128, 70, ["pad1"], seed=20 + fmt)


def test_attention_decode_masked_fp16_operand_library(be16):
    kc.check_attention_decode_masked(be16, 0, 3, 1, 128, 200, ["early", "tile", "ones"], seed=1)
    kc.check_attention_decode_masked(be16, 3, 3, 1, 128, 200, ["straddle", "pad64", "ones"], seed=2)


def test_attention_f32_masked_and_attn_probs(be):
    kc.check_attention_f32_masked(be, 3, 1, 200, 128, True, ["early", "pad63", "ones"])
    kc.check_attention_f32_masked(be, 2, 2, 70, 64, False, ["singles", "pad1"])
    kc.check_attn_probs(be, "f32", "f32", 2, 1, 200, 128, ["early", "ones"], needle=True)            # the strict prefill
    kc.check_attn_probs(be, "bf16", "bf16", 3, 2, 150, 64, ["tile", "pad64", "singles"], needle=True, seed=1)   # the bf16 prefill
    kc.check_attn_probs(be, "hilo", "hilo", 2, 1, 140, 128, ["straddle", "pad1"], needle=True, seed=2)   # the split prefill
    for kform in ("bf16", "f32", "fp24", "e4m3"):    # a cached decode step: T = 1 at q_pos0, fp32 q
        kc.check_attn_probs(be, "f32", kform, 3, 2, 1, 128, ["early", "pad63", "ones"], q_pos0=199, seed=3)
    for kform in ("bf16", "e4m3"):                   # a continuation: n queries behind P cached keys
        kc.check_attn_probs(be, "bf16", kform, 2, 1, 37, 128, ["tile", "singles"], q_pos0=150, needle=True, seed=4)


def test_splice_greedy_synth(be):
    kc.check_splice(be, 256)
    kc.check_greedy(be, 3, 320)
    kc.check_synth(be)


def test_e4m3_kv_cache_kernels(be):
    """the fp8 weight format's KV cache (1 byte per element): the prefill's writer and the bf16 step's decode attention"""
    kc.check_kv8(be, 3, 2, 128, 140)
    kc.check_kv8(be, 10, 1, 64, 70, T_prefill=33, seed=1)
    kc.check_kv8(be, 1, 2, 128, 400, T_prefill=33, seed=2)   # past one round of the e4m3 rows (384 keys): the early first batch


def test_fused_decode_kernels(be):
    kc.check_gemv_norm_chain(be, 8, 256, 64)
    kc.check_gemv_norm_chain(be, 3, 512, 96, seed=1)
    kc.check_gemv_norm_chain(be, 16, 5120, 32, seed=3)   # 13b row width, all 16 token slots
    kc.check_gemv_norm_chain(be, 5, 288, 64, seed=5)     # odd k-tile count: the last ring slot holds half a pair
    kc.check_gemv_norm_chain(be, 12, 1024, 64, seed=4)
    kc.check_attention_decode_fused(be, 2, 2, 128, 70)
    kc.check_attention_decode_fused(be, 1, 2, 128, 128)
    kc.check_attention_decode_fused(be, 1, 1, 64, 5)
    kc.check_attention_decode_fused(be, 3, 2, 128, 300, per_row=True)   # a position per row, one row inactive (the pool)
    kc.check_attention_decode_fused(be, 2, 1, 64, 40, per_row=True)
    # the first K batch requested behind phase 0's operand loads (pos >= one round of the 8 waves: 256 keys at hd 128, 512 at 64) and
    # the old order on either side of that boundary
    kc.check_attention_decode_fused(be, 2, 1, 128, 256, seed=2)
    kc.check_attention_decode_fused(be, 1, 1, 128, 255, seed=3)
    kc.check_attention_decode_fused(be, 1, 2, 128, 600, seed=4)
    kc.check_attention_decode_fused(be, 1, 1, 64, 520, seed=5)
    kc.check_attention_decode_kv32(be, 2, 1, 128, 300, seed=6)   # the split step's fp32 / fp24 caches past one round (192 keys)
    kc.check_attention_decode_kv32(be, 1, 1, 128, 100, seed=7)
    kc.check_select_embed(be, 3, 320, 256)


def test_device_sampling(be):
    """temperature / top-k / top-p sampling in the select kernel against the HF warper semantics (small vocabulary)."""
    kc.check_sampling(be, 64, 0.7, 0, 1.0, draws=512)
    kc.check_sampling(be, 64, 0.2, 5, 1.0, draws=256)        # serve/cli.py: temperature 0.2 (+ HF's default top_k)
    kc.check_sampling(be, 96, 1.0, 0, 0.6, draws=512)        # serve/chat.py: top_p
    kc.check_sampling(be, 64, 1.3, 12, 0.8, draws=512)
    kc.check_uniform_extremes(be)


def test_strict_fp32_kernels(be):
    kc.check_gemm_f32(be, 70, 72, 40, 3)
    kc.check_gemm_f32(be, 64, 64, 64, 1)
    kc.check_gemm_f32(be, 33, 128, 100, 4, bias=False)
    kc.check_gemm_f32(be, 20, 64, 32, 5, bias=False)
    kc.check_gemm_f32(be, 5, 16, 588, 2)
    kc.check_attention_f32(be, 1, 2, 17, 64, False)
    kc.check_attention_f32(be, 1, 2, 40, 128, True)
    kc.check_attention_f32(be, 2, 2, 1, 128, True, decode_pos=37)
    kc.check_qkv_rope_f32(be, 2, 5, 2, 128, 0)
    kc.check_qkv_rope_f32(be, 1, 1, 2, 64, 11)


@pytest.mark.parametrize("B,T,H,K,bias,ws,f8,kv8", QKV_CASES)
def test_gemm_qkv_fused_epilogue(be, B, T, H, K, bias, ws, f8, kv8):
    kc.check_gemm_qkv_fused(be, B, T, H, K, bias=bias, ws_mb=ws, f8=f8, kv8=kv8)


@pytest.mark.parametrize("B,T,H,K,bias,ws,f8,kv8", [c for c in QKV_CASES if not c[6]] + [(2, 37, 2, 128, False, 1, False, True)])
def test_gemm_qkv_fused_epilogue_padded_rows(be, B, T, H, K, bias, ws, f8, kv8):
    """token rows of stride K + 64 (NaN pad, tight end): the clamped padded token rows of a sample length off the 32-token grid
    address through lda too"""
    kc.check_gemm_qkv_fused(be, B, T, H, K, bias=bias, ws_mb=ws, f8=f8, kv8=kv8, lda_pad=64)


def test_gemm_qkv_fused_epilogue_splitk_round(be):
    """more than one round of 256 tiles with a short last round: K-slices + the QKV fix-up launch (2 x 640 tokens, H = 22:
    5 x 66 = 330 tiles -> 74 remainder tiles in 3 slices)"""
    kc.check_gemm_qkv_fused(be, 2, 630, 22, 192, ws_mb=64)


def test_alternate_kernel_variants(be):
    """Every GEMM case above again with the bf16 8-phase kernel forced onto every size (vck_set_gemm_force_8phase): small, ragged
    and 1-3 k-tile problems, the split-K rounds of the bf16 and the e4m3 form, the fused QKV epilogue against that GEMM."""
    be.lib.vck_set_gemm_force_8phase(1)
    be.forced_8phase = True
    try:
        for case in GEMM_CASES:
            test_gemm(be, *case)
            test_gemm_padded_rows(be, *case)
        kc.check_rmsnorm(be, 6, 4096)      # rmsnorm_ld -> gemm(lda = D + 64) on the 8-phase kernel
        test_gemm_splitk_remainder_round(be)
        for case in GEMM_F8_CASES:
            test_gemm_f8(be, *case)
        test_gemm_f8_splitk_remainder_round(be)
        for case in QKV_CASES:
            test_gemm_qkv_fused_epilogue(be, *case)
            if not case[6]:
                test_gemm_qkv_fused_epilogue_padded_rows(be, *case)
        test_gemm_qkv_fused_epilogue_splitk_round(be)
    finally:
        be.lib.vck_set_gemm_force_8phase(0)
        be.forced_8phase = False


def test_fp16_operand_library_new_call_forms(be16):
    """one case of each strided / offset call form on the -DVC_F16 build (its NaN pad pattern, its conversions)"""
    assert be16.lib.vc_operand_format() == 1
    kc.check_gemm(be16, 200, 136, 128, 0, True, lda_pad=64, ldw_pad=16, path="dma")
    be16.lib.vck_set_gemm_force_8phase(1)
    try:
        kc.check_gemm(be16, 70, 264, 192, 1, True, lda_pad=64, path="8phase")
    finally:
        be16.lib.vck_set_gemm_force_8phase(0)
    kc.check_gemm_qkv_fused(be16, 2, 70, 2, 192, bias=True, lda_pad=64)
    kc.check_gemm_f8(be16, 100, 144, 128, 0, path="8phase")
    kc.check_rmsnorm(be16, 6, 4096)
    kc.check_qkv_split_at_offset(be16, 1, 21, 2, 128, 75, False)
    kc.check_qkv_split_at_offset(be16, 2, 5, 2, 128, 130, True)


@pytest.mark.parametrize("M,N,K,epi,norm,G,ks", [
    (5, 64, 256, 0, True, 8, 0), (13, 48, 320, 2, True, 16, 0), (29, 96, 576, 3, True, 32, 0), (32, 64, 1024, 1, True, 32, 4),
    (21, 80, 384, 2, True, 24, 2), (8, 64, 256, 3, True, 8, 0), (1, 16, 64, 1, False, 8, 0), (16, 48, 320, 2, False, 16, 0),
    (24, 64, 512, 0, False, 24, 3)])
def test_gemv_wg(be, M, N, K, epi, norm, G, ks):
    """the workgroup-shared-activation decode GEMV of precision mode "split": all row counts (1..4 activation pieces), epilogues,
    both planes in one weight pass, K-slices over workgroups"""
    kc.check_gemv_wg(be, M, N, K, epi, norm, G, ks)


@pytest.mark.parametrize("N,K,epi,norm,rows", [(16 * 700, 192, 0, True, (5, 13, 19, 32)), (16 * 767, 128, 0, True, (8, 29)),
                                               (16 * 900, 128, 0, False, (8, 16, 19, 32)), (16 * 1376, 128, 3, True, (3, 16, 24, 29)),
                                               (16 * 1727, 64, 3, True, (8, 9, 17, 32))])
def test_gemv_wide_geometry(be, N, K, epi, norm, rows):
    """the one-workgroup-per-CU geometries (3 / 4 / 6 / 7 tiles per workgroup) give the pair geometry's bits"""
    kc.check_gemv_wide(be, N, K, epi, rows, norm)


def test_gemv_plan_matches_recorded(be):
    """The decode GEMV's launch geometry — which kernel instance, how many K-slices and workgroups, or a refusal — for every call of
    tests/golden/gemv_plan.npz is what the launcher chose when the rows were recorded.  Every geometry computes the same bits, so no
    numerical test sees a threshold, ring depth or table cell of decode.hip's gemv_plan move: this one does.  The rows: every
    tile-count class boundary x 1 / 8 / 9 / 16 / 17 / 24 / 25 / 32 rows x bf16 and W8A16 weights x the (K, epilogue) pairs of the 7b
    and 13b matrices, with and without the split-K buffers; the split step (G = 8 / 16 / 32, with and without a weight lo plane) at
    the 7b and 13b shapes; every non-default vck_set_gemv_variant / vck_set_gemv_wide value at the 7b shapes.  A deliberate geometry
    change regenerates the rows it touches (the `plans` row of each affected call, from vck_gemv_plan) in the same commit and cites
    the measurement that justifies it, next to the table cell it changes."""
    import os
    import numpy as np
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_plan.npz"))
    calls, plans = g["calls"], g["plans"]
    assert list(g["plan_columns"][1:]) == list(kc.GEMV_PLAN_FIELDS) and len(calls) == len(plans) > 5000
    wrong = []
    try:
        for call, want in zip(calls.tolist(), plans.tolist()):
            M, N, K, epi, fp8, G, ks, has_sk, sk_floats, sk_n, wlo, variant, wide = call
            be.lib.vck_set_gemv_variant(variant)
            be.lib.vck_set_gemv_wide(wide)
            got = kc.gemv_plan(be, M, N, K, epi, fp8=fp8, G=G, ksplit=ks, sk=(sk_floats, sk_n) if has_sk else None, wlo=wlo)
            refused, want = want[0] != 0, dict(zip(kc.GEMV_PLAN_FIELDS, want[1:]))
            if (got is None) != refused or (got is not None and got != want):
                wrong.append((dict(zip(g["call_columns"].tolist(), call)), "refused" if refused else want, got))
    finally:
        be.lib.vck_set_gemv_variant(-1)
        be.lib.vck_set_gemv_wide(-1)
    assert not wrong, f"{len(wrong)} of {len(calls)} calls plan differently from the recording; the first (call, recorded, now): {wrong[:3]}"


@pytest.mark.parametrize("N,K,epi,norm,rows,ks", [(16 * 13, 576, 0, False, (5, 16, 19, 32), 0), (16 * 13, 576, 2, False, (8, 29), 2),
                                                  (16 * 7, 1024, 1, False, (13, 32), 4), (16 * 12, 320, 3, False, (8, 24), 0),
                                                  (16 * 13, 576, 2, True, (8, 32), 3), (16 * 6, 256, 0, True, (16, 17), 0)])
def test_gemv_wg_six_waves_per_workgroup(be, N, K, epi, norm, rows, ks):
    """six tiles per workgroup (the balanced geometry of 7b qkv / gate-up and 13b o / down in precision mode split): the four-wave
    geometry's bits without the folded norm, its values within the float64 tolerance with it; ragged last workgroup, K-slices, every epilogue"""
    kc.check_gemv_wg_six_waves(be, N, K, epi, rows, norm, ks)


def test_gemv_wg_chooses_six_waves_for_unbalanced_launches(be):
    """1376 tiles (7b gate / up): 344 four-wave workgroups would leave 88 CUs with two — the launcher takes six waves (230
    workgroups); the result against float64 as for every other geometry"""
    kc.check_gemv_wg(be, 29, 16 * 1376, 128, 3, True, 32, 0)
    kc.check_gemv_wg(be, 8, 16 * 1376, 128, 3, False, 8, 0, seed=1)


@pytest.mark.parametrize("N,K,epi,G,ks", [(64, 512, 0, True, 0), (48, 1024, 1, True, 4), (64, 256, 3, True, 0), (32, 512, 2, True, 2)])
def test_gemv_wg_rows_agree(be, N, K, epi, G, ks):
    kc.check_gemv_wg_rows_agree(be, N, K, epi, True, G, ks)
