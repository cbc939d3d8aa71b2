"""W8A16 and W4A16 weight formats of the decode GEMV (BASELINE.json configs[4], "fp8 weights"; MXFP4 below) — host restatement.

The device quantiser (`quantize_fp8_kernel`, csrc/decode.hip) runs at `vc_model_finalize`; this module states the same
arithmetic in numpy so checkpoints can be inspected / pre-quantised on the host and so the tests can hand the CPU
reference restatement exactly the effective weights the GPU computes with:

  per output row n of W [N, K]:   s_n = 2^e, e = the smallest integer with max|W[n]| <= 448 * 2^e
                                  q   = e4m3fn( W[n] / s_n )      round-to-nearest-even, saturating at +-448
                                  W_eff[n] = q * s_n               (exactly representable in bf16)

The reference's own reduced-precision switch is `load_8bit` (`vcoder_llava/model/builder.py:31-33`, bitsandbytes
LLM.int8); fp8-e4m3 with a power-of-two row scale is the MI355X-native counterpart: the scale is exact in every
format on the path, so prefill (bf16 MFMA over W_eff) and decode (bytes widened in registers, scale applied to the
fp32 accumulator) see identical weights.
"""
from __future__ import annotations

import numpy as np

E4M3_MAX = 448.0


def e4m3_encode(x: np.ndarray) -> np.ndarray:
    """float32 -> OCP e4m3fn bytes (RNE, saturating).  Mirrors `f2fp8` in csrc/vc_device.h."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    sign = ((u >> 24) & 0x80).astype(np.uint32)
    a = np.abs(x)
    sub = np.rint(np.minimum(a, np.float32(1.0)) * np.float32(512.0)).astype(np.uint32)
    e = ((u >> 23) & 0xFF).astype(np.int32) - 127
    m = ((u & 0x007FFFFF) | 0x3F800000).astype(np.uint32).view(np.float32)
    code = ((np.clip(e, -6, 8) + 7).astype(np.uint32) << 3) + np.rint((m - np.float32(1.0)) * np.float32(8.0)).astype(np.uint32)
    code = np.minimum(code, 0x7E)
    out = np.where(a < np.float32(0.015625), sub, code)
    out = np.where(a < np.float32(448.0), out, 0x7E)
    return (sign | out).astype(np.uint8)


def e4m3_decode(b: np.ndarray) -> np.ndarray:
    b = np.asarray(b, dtype=np.uint8).astype(np.uint32)
    e = (b >> 3) & 15
    m = b & 7
    normal = (((e + 120) << 23) | (m << 20)).astype(np.uint32).view(np.float32)
    mag = np.where(e == 0, m.astype(np.float32) * np.float32(2.0 ** -9), normal)
    return np.where(b & 0x80, -mag, mag).astype(np.float32)


def row_scales(W: np.ndarray) -> np.ndarray:
    """Per-row power-of-two scale: the smallest 2^e with max|row| <= 448 * 2^e (1.0 for an all-zero row)."""
    amax = np.abs(np.asarray(W, dtype=np.float32)).max(axis=1)
    u = amax.view(np.uint32)
    e = (u >> 23).astype(np.int32) - 127 - np.where((u & 0x007FFFFF) <= 0x00600000, 8, 7)
    e = np.where(amax > 0, e, 0)
    return np.ldexp(np.float32(1.0), e).astype(np.float32)


def quantize_rows(W: np.ndarray):
    """W [N, K] (bf16-valued float32) -> (q uint8 [N, K], scale float32 [N], W_eff float32 [N, K])."""
    W = np.asarray(W, dtype=np.float32)
    s = row_scales(W)
    q = e4m3_encode(W / s[:, None])
    return q, s, e4m3_decode(q) * s[:, None]


def pack_supertiles(q: np.ndarray) -> np.ndarray:
    """q [N, K] bytes -> the decode GEMV's order [N/16][K/64][64 lanes][16 B], lane = n%16 + 16*((k%64)/16)."""
    N, K = q.shape
    t = q.reshape(N // 16, 16, K // 64, 4, 16)  # [nt][n%16][st][g][byte]
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1, 4)).reshape(-1)


# decoder state-dict keys that the W8A16 format quantises (HF names; q/k/v are quantised row-wise, so the fused
# [3D, D] device matrix equals the three matrices quantised separately — likewise gate/up)
QUANTIZED_SUFFIXES = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                      "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")


# ---- W4A16: MXFP4 (OCP e2m1 elements, one E8M0 power-of-two scale per 32 consecutive k of a row) ---------------------------------
# Host restatement of `quantize_mxfp4_kernel` (csrc/decode.hip):
#   per row n and block b of 32 consecutive k:  e = the smallest integer with max|W[n, 32b:32b+32]| <= 6 * 2^e, >= MX_MIN_E
#                                               (0 for an all-zero block), stored as the byte e + 127
#                                               q = e2m1(W / 2^e)   round to nearest, ties to the even code; |W / 2^e| <= 6
#                                               W_eff = value(q) * 2^e
# Every W_eff is exactly representable in bf16 and — the clamp keeps 0.5 * 2^e a normal fp16 — in fp16, for weights below fp16's
# range.  This is not bitsandbytes NF4 (fp32 absmax x a non-dyadic codebook), which has no such property.
MX_BLOCK = 32
MX_MIN_E = -13
E2M1_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)


def e2m1_encode(x: np.ndarray) -> np.ndarray:
    """float32 (|x| <= 6) -> e2m1 codes 0..15 (sign in bit 3, copied from the input).  Mirrors `f2fp4` in csrc/vc_device.h."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x)
    f = np.float32
    code = ((a > f(0.25)).astype(np.uint8) + (a >= f(0.75)) + (a > f(1.25)) + (a >= f(1.75)) + (a > f(2.5)) + (a >= f(3.5)) + (a > f(5.0)))
    sign = ((x.view(np.uint32) >> 28) & 8).astype(np.uint8)
    return (sign | code.astype(np.uint8)).astype(np.uint8)


def e2m1_decode(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c, dtype=np.uint8)
    mag = E2M1_VALUES[c & 7]
    return np.where(c & 8, -mag, mag).astype(np.float32)


def mx_block_scales(W: np.ndarray) -> np.ndarray:
    """W [N, K] -> the block exponents e [N, K/32] (int32); the stored E8M0 byte is e + 127."""
    W = np.asarray(W, dtype=np.float32)
    N, K = W.shape
    amax = np.ascontiguousarray(np.abs(W).reshape(N, K // MX_BLOCK, MX_BLOCK).max(axis=2))
    u = amax.view(np.uint32)
    e = (u >> 23).astype(np.int32) - 127 - np.where((u & 0x007FFFFF) <= 0x00400000, 2, 1)
    return np.where(amax > 0, np.maximum(e, MX_MIN_E), 0).astype(np.int32)


def quantize_blocks_mxfp4(W: np.ndarray):
    """W [N, K] (values of the library's 16-bit format as float32; K % 128 == 0) ->
    (q uint8 [N, K/2]: element k even in the low nibble, k + 1 in the high one; scale uint8 [N, K/32]: E8M0 bytes; W_eff float32 [N, K])."""
    W = np.asarray(W, dtype=np.float32)
    N, K = W.shape
    assert K % 128 == 0, "MXFP4 needs K divisible by 128"
    e = mx_block_scales(W)
    s = np.repeat(np.ldexp(np.float32(1.0), e).astype(np.float32), MX_BLOCK, axis=1)
    codes = e2m1_encode(W / s)
    w_eff = e2m1_decode(codes) * s
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return q, (e + 127).astype(np.uint8), w_eff


def pack_w4(q: np.ndarray, scale: np.ndarray):
    """(q [N, K/2], scale [N, K/32]) -> the device layout of the W4A16 GEMV: nibbles [N/16][K/128][64 lanes][16 B] and scale bytes
    [N/16][K/128][64 lanes], lane = n%16 + 16*((k%128)/32) — a lane's 16 bytes are one MX block of one output row."""
    N, K2 = q.shape
    K = K2 * 2
    qt = q.reshape(N // 16, 16, K // 128, 4, 16)        # [nt][n%16][st][g][byte]
    st = scale.reshape(N // 16, 16, K // 128, 4)        # [nt][n%16][st][g]
    return (np.ascontiguousarray(qt.transpose(0, 2, 3, 1, 4)).reshape(-1), np.ascontiguousarray(st.transpose(0, 2, 3, 1)).reshape(-1))


def effective_state_dict(sd: dict, fmt: str = "w8a16") -> dict:
    """The state dict the device computes with under W8A16 (default; 'fp8' has the same weights) or, fmt='w4a16', under MXFP4:
    decoder linears replaced by their dequantised values."""
    if fmt not in ("w8a16", "fp8", "w4a16"):
        raise ValueError(f"no effective weights for format '{fmt}'")
    quantize = (lambda a: quantize_blocks_mxfp4(a)[2]) if fmt == "w4a16" else (lambda a: quantize_rows(a)[2])
    out = {}
    for k, v in sd.items():
        if k.startswith("model.layers.") and k.endswith(QUANTIZED_SUFFIXES):
            arr = v.detach().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)
            w_eff = quantize(arr)
            if hasattr(v, "detach"):
                import torch

                out[k] = torch.from_numpy(w_eff).to(v.dtype)
            else:
                out[k] = w_eff
        else:
            out[k] = v
    return out
