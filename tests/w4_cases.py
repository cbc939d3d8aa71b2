"""W4A16 (MXFP4 decoder weights) cases shared by the CPU-emulator tests (tests/test_w4_emu.py) and the `-m gpu` tests
(tests/test_gpu_w4.py), written once against the backends of kernel_cases.

The format's own error is not part of any bar here: vcoder_amd/quant.py restates the quantiser bit for bit, so every reference is
computed on the effective weights W_eff = q * 2^e and the tolerances are those of the bf16 / W8A16 paths."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

import cpu_ref
import e2e_cases
import extend_cases as xc
import kernel_cases as kc
from kernel_cases import _call, _rstd, bf16_round, rel_err
from vcoder_amd import quant, synth
from vcoder_amd.engine import HipEngine

GEMV_FORM_W4 = 3
# every gemv_w4_kernel instance of the library (decode.hip VC_GEMV_W4_INSTANCES): (tiles per workgroup, ring slots, activation pieces)
W4_INSTANCES = {(1, 4, 1), (1, 3, 2), (1, 2, 3), (1, 2, 4), (2, 3, 1), (2, 2, 2), (2, 2, 3), (2, 2, 4), (4, 5, 1), (4, 3, 2), (4, 3, 3), (4, 2, 4)}


# (M, N, K, nt): K = 128 one super-tile (most waves idle), 384 fewer super-tiles than waves, 1408 = 11, no multiple of the wave count;
# N = 16 / 80 ragged last tile groups for NT = 2, 4; M over the four piece counts and both row groups
GEMV_CASES = [(1, 16, 128, 0), (8, 80, 384, 1), (9, 80, 128, 2), (16, 16, 384, 4), (17, 80, 384, 4), (29, 80, 128, 1), (32, 80, 384, 2),
              (1, 80, 1408, 4), (17, 16, 1408, 1), (9, 80, 384, 4), (29, 80, 384, 4), (1, 80, 384, 2), (24, 16, 128, 2), (32, 16, 128, 1),
              (9, 16, 128, 1)]


def op_round(be, x):
    """x rounded to the library's 16-bit operand format, as fp32"""
    return kc._op_decode(kc._op_bits(x, be.operands), be.operands)


def w4_matrix(rng, N, K, be=None):
    """check_gemv_fp8's recipe moved to blocks: block magnitudes over ~10 octaves, one all-zero block, one outlier that flushes the
    rest of its block to zero, one block under the scale clamp (2^-13)"""
    W = rng.randn(N, K) * 0.05 * np.repeat(np.exp2(rng.randint(-6, 4, size=(N, K // 32))), 32, axis=1)
    n0, b0 = rng.randint(N), rng.randint(K // 32)
    W[n0, 32 * b0:32 * b0 + 32] = 0.0
    n1, b1 = (n0 + 1) % N, rng.randint(K // 32)
    W[n1, 32 * b1 + rng.randint(32)] = 37.0
    n2, b2 = (n0 + 2) % N, rng.randint(K // 32)
    W[n2, 32 * b2:32 * b2 + 32] = rng.randn(32) * 2.0 ** -16
    W = bf16_round(W) if be is None else op_round(be, W)
    return W, (n0, b0), (n1, b1), (n2, b2)


def _u8(be, a):
    return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def quantize_on_device(be, W):
    """-> (device W (rewritten), device nibbles, device scale bytes)"""
    N, K = W.shape
    Wb, Wq, sc = be.bf16(W), be.zeros((N * K // 2,), "u8"), be.zeros((N * K // 32,), "u8")
    _call(be, "vck_quantize_mxfp4", Wb, Wq, sc, N, K)
    return Wb, Wq, sc


def check_quantizer(be, N, K, seed=0):
    """device scales, nibbles (through pack_w4) and the rewritten matrix are array_equal to vcoder_amd/quant.py"""
    rng = np.random.RandomState(seed)
    W, zero, outlier, tiny = w4_matrix(rng, N, K, be)
    q, s, w_eff = quant.quantize_blocks_mxfp4(W)
    assert s[zero] == 127 and not w_eff[zero[0], 32 * zero[1]:32 * zero[1] + 32].any()
    blk = w_eff[outlier[0], 32 * outlier[1]:32 * outlier[1] + 32]
    assert np.count_nonzero(blk) == 1 and blk.max() == 32.0   # 37 -> 4 * 2^3; the rest of the block is flushed to zero
    assert s[tiny] == 127 + quant.MX_MIN_E
    Wb, Wq, sc = quantize_on_device(be, W)
    pq, ps = quant.pack_w4(q, s)
    assert np.array_equal(_u8(be, sc), ps), "E8M0 scale bytes differ from quant.mx_block_scales / pack_w4"
    assert np.array_equal(_u8(be, Wq), pq), "e2m1 nibbles differ from quant.e2m1_encode / pack_w4"
    assert np.array_equal(be.host_f32(Wb), w_eff), "effective-weight rewrite differs"
    assert np.array_equal(bf16_round(w_eff), w_eff) and np.array_equal(w_eff.astype(np.float16).astype(np.float32), w_eff)


def w4_plan(be, M, N, K, epi, G=0, ksplit=0, sk=False):
    """what vck_gemv_w4 would launch -> dict, or None where the plan refuses the call"""
    out = (ctypes.c_int * 7)()
    if be.lib.vck_gemv_w4_plan(M, N, K, epi, G, ksplit, int(sk), out) != 0:
        return None
    return dict(zip(("form", "waves", "nt", "r", "xp", "ksplit", "workgroups"), list(out)))


def _gemv_w4(be, X, Wq, sc, out, ssq_in, ssq_out, xg_w, xg_out, npart, M, N, K, ldo, epi, sk=None, ksplit=0):
    be.lib.vck_gemv_w4(be.ptr(X), be.ptr(Wq), be.ptr(sc), be.ptr(out), be.ptr(ssq_in), be.ptr(ssq_out), be.ptr(xg_w), be.ptr(xg_out),
                       ctypes.c_int(npart), ctypes.c_float(1e-5), be.ptr(sk[0]) if sk else None, be.ptr(sk[1]) if sk else None,
                       ctypes.c_int(ksplit), M, N, K, ldo, epi, None)
    be.sync()


class force_nt:
    """tiles per workgroup of the W4A16 kernel for the launches inside (0 = by the tile count)"""

    def __init__(self, be, nt):
        self.be, self.nt = be, nt

    def __enter__(self):
        self.be.lib.vck_set_gemv_w4_nt(self.nt)

    def __exit__(self, *a):
        self.be.lib.vck_set_gemv_w4_nt(0)


_seen = {}   # backend name -> the (nt, r, xp) instances the GEMV cases launched so far


def check_gemv(be, M, N, K, epi, norm=False, nt=0, seed=0):
    """the nibble-streaming GEMV against X @ W_eff^T in float64, check_gemv_fp8's bars; the RESID form also publishes xg_out / ssq_out.
    nt: force that many tiles per workgroup (0: the plan's own choice).  -> (rel err, the plan taken)"""
    rng = np.random.RandomState(seed)
    W = w4_matrix(rng, N, K, be)[0]
    w_eff = quant.quantize_blocks_mxfp4(W)[2]
    Wb, Wq, sc = quantize_on_device(be, W)
    npart = (max(K, N) // 16 + 15) // 16 * 16
    ssq, scale_rows = None, 1.0
    X = op_round(be, rng.randn(M, K))
    if norm:
        x32 = (rng.randn(M, K) * 1.5).astype(np.float32)
        g = (rng.rand(K) + 0.5).astype(np.float32)
        X = op_round(be, x32 * g)
        part = np.zeros((32, npart), np.float32)
        part[:M, : npart // 2] = ((x32.astype(np.float64) ** 2).sum(-1) / (npart // 2))[:, None]
        ssq = be.f32(part)
        scale_rows = _rstd(x32)
    t = torch.from_numpy((X.astype(np.float64) @ w_eff.T.astype(np.float64)) * scale_rows).float()
    xg_w = xg_out = ssq_out = None
    if epi == 0:
        out = be.zeros((M, N), "bf16")
    elif epi == 1:
        out = be.zeros((M, N), "f32")
    elif epi == 2:
        r0 = rng.randn(M, N).astype(np.float32)
        out = be.f32(r0)
        t = t + torch.from_numpy(r0)
        gw = (rng.rand(N) + 0.5).astype(np.float32)
        xg_w, xg_out, ssq_out = be.f32(gw), be.zeros((M, N), "bf16"), be.zeros((M, npart), "f32")
    else:
        out = be.zeros((M, N // 2), "bf16")
        t = torch.nn.functional.silu(t[:, 0::2]) * t[:, 1::2]
    Xd = be.bf16(X)
    with force_nt(be, nt):
        plan = w4_plan(be, M, N, K, epi)
        assert plan is not None and plan["form"] == GEMV_FORM_W4 and plan["waves"] == 4 and plan["xp"] == (M + 7) // 8 and plan["ksplit"] == 1, plan
        assert (plan["nt"], plan["r"], plan["xp"]) in W4_INSTANCES, plan
        assert nt == 0 or plan["nt"] == nt, plan
        _gemv_w4(be, Xd, Wq, sc, out, ssq, ssq_out, xg_w, xg_out, npart, M, N, K, N // 2 if epi == 3 else N, epi)
    _seen.setdefault(be.name + be.operands, set()).add((plan["nt"], plan["r"], plan["xp"]))
    got = be.host_f32(out)
    e = rel_err(got, t.numpy())
    print(f"gemv_w4 M{M} N{N} K{K} epi{epi} norm{int(norm)} nt{plan['nt']} r{plan['r']} [{be.operands}]: rel err {e:.3e}")
    tol = 2 ** -8 if epi in (0, 3) else 2e-5
    assert e < tol, f"gemv_w4 M{M} N{N} K{K} epi{epi} norm{norm} plan {plan}: rel err {e}"
    if epi == 2:   # the producer side, as the ring tests check it (kernel_cases.check_gemv_norm_chain / check_gemv_split)
        xg = be.host_f32(xg_out).astype(np.float64)
        e2 = rel_err(xg, got.astype(np.float64) * gw)
        assert e2 < 2 ** -8, f"gemv_w4 xg_out: {e2}"
        so = be.host_f32(ssq_out)[:, : N // 16].astype(np.float64).sum(-1)
        assert np.abs(so / (got.astype(np.float64) ** 2).sum(-1) - 1).max() < 1e-5, "gemv_w4 ssq_out"
    return e, plan


def check_true_shape(be, N, K, epi, seed=0):
    """one decoder linear of the 7b / 13b models at M = 1 and M = 32, one launch each over one quantised matrix.  The reference's
    matrix is the device quantiser's own rewrite (its equality with quant.py is check_quantizer's, at small shapes: restating 140 M
    elements in numpy would take longer than everything else here); rows of W repeat every 512 with another octave per row."""
    rng = np.random.RandomState(seed)
    base = rng.randn(512, K) * 0.05
    W = np.tile(base, (N // 512, 1)) * np.exp2(rng.randint(-6, 4, size=(N, 1)))
    Wb, Wq, sc = quantize_on_device(be, bf16_round(W))
    w_eff = be.host_f32(Wb).astype(np.float64)
    norm = epi in (0, 3)
    npart = (max(K, N) // 16 + 15) // 16 * 16
    for M in (1, 32):
        x32 = (rng.randn(M, K) * 1.5).astype(np.float32)
        X = bf16_round(x32 * (rng.rand(K) + 0.5).astype(np.float32))
        part = np.zeros((32, npart), np.float32)
        part[:M, : npart // 2] = ((x32.astype(np.float64) ** 2).sum(-1) / (npart // 2))[:, None]
        t = torch.from_numpy((X.astype(np.float64) @ w_eff.T) * (_rstd(x32) if norm else 1.0)).float()
        if epi == 0:
            out = be.zeros((M, N), "bf16")
        elif epi == 2:
            r0 = rng.randn(M, N).astype(np.float32)
            out = be.f32(r0)
            t = t + torch.from_numpy(r0)
        else:
            out = be.zeros((M, N // 2), "bf16")
            t = torch.nn.functional.silu(t[:, 0::2]) * t[:, 1::2]
        plan = w4_plan(be, M, N, K, epi)
        assert plan is not None and (plan["nt"], plan["r"], plan["xp"]) in W4_INSTANCES and plan["xp"] == (M + 7) // 8, plan
        _gemv_w4(be, be.bf16(X), Wq, sc, out, be.f32(part) if norm else None, None, None, None, npart, M, N, K, N // 2 if epi == 3 else N, epi)
        e = rel_err(be.host_f32(out), t.numpy())
        print(f"gemv_w4 true shape M{M} N{N} K{K} epi{epi} plan {plan}: rel err {e:.3e}")
        assert e < (2 ** -8 if epi in (0, 3) else 2e-5), f"gemv_w4 M{M} N{N} K{K} epi{epi}: rel err {e}"


def instances_seen(be):
    return _seen.get(be.name + be.operands, set())


def check_rows_agree(be, N, K, epi, norm=True, ksplit=0, nts=(0,), M=29, seed=0):
    """kernel_cases.check_gemv_rows_agree_across_variants for the W4A16 kernel: the rows of one M-row launch are bit-equal to the
    same rows served by launches of <= 8 and <= 16 rows — under every tile geometry in `nts` (the K partition does not depend on the
    rows, NT or the ring depth), with ksplit K-slices where asked."""
    rng = np.random.RandomState(seed)
    npart = (K // 16 + 15) // 16 * 16
    X = bf16_round(rng.randn(32, K))
    W = w4_matrix(rng, N, K)[0]
    w_eff = quant.quantize_blocks_mxfp4(W)[2]
    _, Wq, sc = quantize_on_device(be, W)
    ssq = np.zeros((32, npart), np.float32)
    ssq[:, : K // 16] = rng.rand(32, K // 16).astype(np.float32) + 0.5
    No = N // 2 if epi == 3 else N
    esz = {0: "bf16", 1: "f32", 2: "f32", 3: "bf16"}[epi]
    r0 = rng.randn(32, No).astype(np.float32)
    sk = (be.zeros((max(ksplit, 1) * (N // 16) * 2 * 256,), "f32"), be.zeros((N // 16 * 2,), "i32")) if ksplit else None

    def run(row0, rows, nt):
        out = be.f32(r0[row0:row0 + rows].copy()) if epi == 2 else be.zeros((rows, No), esz)
        Xd = be.bf16(X[row0:row0 + rows])
        sd = be.f32(ssq[row0:row0 + rows]) if norm else None
        with force_nt(be, nt):
            plan = w4_plan(be, rows, N, K, epi, ksplit=ksplit, sk=bool(sk))
            assert plan is not None and plan["ksplit"] == max(ksplit, 1) and (nt == 0 or plan["nt"] == nt), plan
            _gemv_w4(be, Xd, Wq, sc, out, sd, None, None, None, npart, rows, N, K, No, epi, sk=sk, ksplit=ksplit)
        return kc.raw_bits(out), be.host_f32(out)

    big_bits, big = run(0, M, nts[0])
    for nt in nts:
        for (row0, rows) in [(0, 8), (8, 8), (16, 8), (24, M - 24), (0, 16), (16, M - 16)]:
            bits, _ = run(row0, rows, nt)
            assert np.array_equal(big_bits[row0:row0 + rows], bits), \
                f"rows {row0}..{row0 + rows - 1} of the {M}-row launch differ from the {rows}-row launch (nt {nt}, ksplit {ksplit})"
    ref = X[:M].astype(np.float64) @ w_eff.T.astype(np.float64)
    if norm:
        ref = ref / np.sqrt(ssq[:M, : K // 16].sum(-1, keepdims=True) / K + 1e-5)
    if epi == 3:
        t = torch.from_numpy(ref).float()
        ref = (torch.nn.functional.silu(t[:, 0::2]) * t[:, 1::2]).numpy()
    if epi == 2:
        ref = ref + r0[:M]
    e = rel_err(big[:M], ref)
    assert e < (2 ** -8 if epi in (0, 3) else 2e-5), f"gemv_w4 M={M} N{N} K{K} epi{epi}: rel err {e}"


def check_ksplit_refused_without_buffers(be):
    """split-K either works (check_rows_agree) or is refused by the plan: never dropped silently"""
    assert w4_plan(be, 8, 32, 256, 1, ksplit=2, sk=False) is None
    assert w4_plan(be, 8, 32, 256, 1, ksplit=3, sk=True) is None          # more slices than super-tiles
    assert w4_plan(be, 8, 32, 256, 1, G=8, ksplit=2, sk=True) is None     # no hand-off in split mode
    assert w4_plan(be, 8, 32, 192, 1) is None                             # K % 128
    assert w4_plan(be, 8, 32, 256, 1, ksplit=2, sk=True)["ksplit"] == 2


def check_gemv_split(be, M, N, K, epi, norm=True, seed=0):
    """kernel_cases.check_gemv_split(..., fp8=True) for the W4A16 kernel: stacked hi / lo rows of X (G = 8 for M <= 8, else 16) against
    the float64 product of the fp32 rows with W_eff, the same bars."""
    rng = np.random.RandomState(seed)
    G = 8 if M <= 8 else 16
    npart = (max(K, N) // 16 + 15) // 16 * 16
    Xf = rng.randn(M, K).astype(np.float32)
    hi, lo = kc.split_hi_lo(Xf)
    X = np.zeros((2 * G, K), np.float32)
    X[:M], X[G:G + M] = hi, lo
    X[M:G] = 7.0   # rows of the group beyond M must not be read into any result
    W = w4_matrix(rng, N, K)[0]
    w_eff = quant.quantize_blocks_mxfp4(W)[2]
    _, Wq, sc = quantize_on_device(be, W)
    ssq = np.zeros((16, npart), np.float32)
    ssq[:, : K // 16] = rng.rand(16, K // 16).astype(np.float32) + 0.5
    ref = Xf.astype(np.float64) @ w_eff.T.astype(np.float64)
    if norm:
        ref = ref / np.sqrt(ssq[:M, : K // 16].astype(np.float64).sum(-1, keepdims=True) / K + 1e-5)
    No = N // 2 if epi == 3 else N
    gw = (rng.rand(N).astype(np.float32) + 0.5) if epi == 2 else None
    if epi == 3:
        t = torch.from_numpy(ref)
        ref = (torch.nn.functional.silu(t[:, 0::2]) * t[:, 1::2]).numpy()
    r0 = rng.randn(16, No).astype(np.float32)
    if epi == 2:
        ref = ref + r0[:M]
        out = be.f32(r0.copy())
    elif epi == 1:
        out = be.zeros((16, No), "f32")
    else:
        out = be.zeros((2 * G, No), "bf16")
    xg_out = be.zeros((2 * G, N), "bf16") if epi == 2 else None
    ssq_out = be.zeros((16, npart), "f32") if epi == 2 else None
    Xd, ssqd, gwd = be.bf16(X), (be.f32(ssq) if norm else None), (be.f32(gw) if gw is not None else None)
    plan = w4_plan(be, M, N, K, epi, G=G)
    assert plan is not None and plan["form"] == GEMV_FORM_W4 and plan["xp"] == (G + M + 7) // 8, plan
    be.lib.vck_gemv_w4_split(be.ptr(Xd), be.ptr(Wq), be.ptr(sc), be.ptr(out), be.ptr(ssqd), be.ptr(ssq_out), be.ptr(gwd), be.ptr(xg_out),
                             ctypes.c_int(npart), ctypes.c_float(1e-5), M, N, K, No, epi, G, None)
    be.sync()
    o = be.host_f32(out).astype(np.float64)
    got = (o[:M] + o[G:G + M]) if epi in (0, 3) else o[:M]
    e = rel_err(got, ref)
    assert e < 3e-5, f"gemv_w4_split M{M} N{N} K{K} epi{epi}: rel err {e}"
    if epi == 2:
        xg = be.host_f32(xg_out).astype(np.float64)
        e2 = rel_err(xg[:M] + xg[G:G + M], got * gw)
        assert e2 < 2e-5, f"gemv_w4_split xg_out: {e2}"
        so = be.host_f32(ssq_out)[:M, : N // 16].astype(np.float64).sum(-1)
        assert np.abs(so / (got ** 2).sum(-1) - 1).max() < 1e-5
        assert np.array_equal(o[M:], r0[M:].astype(np.float64)), "residual rows beyond M were touched"
    return e


# ---- engine ---------------------------------------------------------------------------------------------------------------------
def make_engine(name, lib, precision="bf16", operands="bf16"):
    """-> (engine with weight format 'w4a16', cfg, inputs, the effective state dict, the fixture).  operands="fp16": lib is (None: the
    product's) -DVC_F16 library"""
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    eng = HipEngine(cfg, lib=lib, operands=operands)
    assert eng.lib.vc_operand_format() == (1 if operands == "fp16" else 0)
    eng.load_synthetic(int(g["seed"]))
    eng.set_weight_format("w4a16")
    eng.finalize()
    if precision != "bf16":
        eng.set_precision(precision)
    sd = synth.synth_state_dict(cfg, int(g["seed"]))
    return eng, cfg, (ids, imgs, segs, deps), quant.effective_state_dict(sd, "w4a16"), g


def check_w4_weights(name, lib=None, n_new=6, split=True, operands="bf16"):
    """e2e_cases.check_fp8_weights for weight format 'w4a16': strict mode against the fp32 oracle on W_eff (TOL_STRICT, bit-exact ids),
    the bf16 path against the bf16-emulating oracle on W_eff while the ids follow, generate_greedy (graph) against the decode_step
    loop, and split mode on the strict bar (the bar of e2e_cases.check_fixture_strict(mode="split")).  operands="fp16": the fp16-operand
    library against the fp16-rounding oracle on the bar of e2e_cases.check_fixture_fp16."""
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    sd = synth.synth_state_dict(cfg, int(g["seed"]))
    sd_eff = quant.effective_state_dict(sd, "w4a16")
    changed = [k for k in sd if not np.array_equal(np.asarray(sd[k]), np.asarray(sd_eff[k]))]
    assert len(changed) == 7 * cfg.num_hidden_layers, "exactly the seven decoder linears per layer are quantised"
    assert all(k.endswith(quant.QUANTIZED_SUFFIXES) for k in changed)
    eng = make_engine(name, lib, operands=operands)[0]
    t = lambda a: None if a is None else torch.from_numpy(a)
    out = {}
    om32 = cpu_ref.OracleModel(cfg, sd_eff, emu_bf16=False)
    ref_ids, ref_logits = om32.generate_greedy(ids.tolist(), t(imgs), t(segs), t(deps), max_new_tokens=n_new, return_logits=True)
    ref_logits = ref_logits.numpy()

    def loop(mode):
        eng.set_precision(mode)
        last, _, _ = eng.prefill(ids, imgs, segs, deps)
        lgs, tok = [last], np.argmax(last, -1).astype(np.int32)
        toks = [tok]
        for _ in range(1, n_new):
            lg, tok = eng.decode_step(tok)
            lgs.append(lg)
            toks.append(tok)
        return np.stack(lgs, 1), np.stack(toks, 1)

    for mode in (("strict", "split") if split else ("strict",)):
        lgs, toks = loop(mode)
        e = float(np.abs(lgs - ref_logits).max())
        print(f"{name} w4a16 {mode}: logits err {e:.3e}")
        assert e < e2e_cases.TOL_STRICT, f"{name}: {mode} logits on w4a16 weights err {e}"
        assert np.array_equal(toks, ref_ids.numpy()), f"{mode} greedy ids on w4a16 weights differ"
        out[mode + "_err"] = e
    om = cpu_ref.OracleModel(cfg, sd_eff, emu_bf16="fp16" if operands == "fp16" else True)
    rel_tol = e2e_cases.REL_TOL_FP16_VS_FP32_REF if operands == "fp16" else e2e_cases.REL_TOL_VS_EMU_ORACLE
    o_ids, o_logits = om.generate_greedy(ids.tolist(), t(imgs), t(segs), t(deps), max_new_tokens=n_new, return_logits=True)
    o_ids, o_logits = o_ids.numpy(), o_logits.numpy()
    lgs, toks = loop("bf16")
    follow = np.cumprod((toks == o_ids).all(0))            # steps at which every row still follows the oracle
    upto = 1 + int(follow[:-1].sum()) if follow[0] else 1    # logits of step s depend on the ids before it
    e = float(np.abs(lgs[:, :upto] - o_logits[:, :upto]).max())
    scale = float(np.abs(o_logits).max())
    print(f"{name} w4a16 {operands} operands: logits err {e / scale:.3e} relative over {upto} steps")
    assert e < rel_tol * scale, f"{name}: w4a16 logits vs the emulating oracle: {e / scale:.2e} relative"
    got = eng.generate_greedy(ids, imgs, segs, deps, max_new_tokens=n_new)
    assert np.array_equal(got, toks), "generate_greedy (graph) disagrees with the decode_step loop"
    out["fast_rel_err"] = e / scale
    out["ids_follow_oracle"] = bool(follow[-1])
    # how far the quantisation moves the model (informational): W_eff logits vs the bf16-weight reference fixture
    out["quantisation_shift"] = float(np.abs(ref_logits[:, 0] - g["step_logits"][:, 0]).max())
    out["quantisation_shift_rel"] = out["quantisation_shift"] / float(np.abs(g["step_logits"][:, 0]).max())
    eng.close()
    return out


def check_extend(name, lib, n):
    """extend(n) against n decode steps of the oracle on W_eff: test_extend_emu's w8a16 bar"""
    eng, cfg, inputs, sd_eff, _ = make_engine(name, lib)
    r = xc.run_sequence(eng, cpu_ref.OracleModel(cfg, sd_eff, emu_bf16=True), inputs, n, np.random.RandomState(n))
    tol = e2e_cases.TOL_VS_FP32_REF
    assert r["extend"] < tol and r["extend_last"] < tol and r["post_steps"] < tol, r
    eng.close()
    return r


def check_refused_hidden_size(lib):
    """a hidden size that is no multiple of 128 is refused at finalize with a readable error"""
    cfg = e2e_cases.tiny_cfg("vcoder_ds")
    cfg.hidden_size, cfg.num_attention_heads = 192, 3
    if hasattr(cfg, "num_key_value_heads"):
        cfg.num_key_value_heads = 3
    eng = HipEngine(cfg, lib=lib)
    eng.load_synthetic(1)
    eng.set_weight_format("w4a16")
    try:
        eng.finalize()
    except Exception as ex:
        assert "128" in str(ex) and "W4A16" in str(ex), str(ex)
    else:
        raise AssertionError("finalize accepted hidden_size 192 under w4a16")
    finally:
        eng.close()


# ---- the features on top: one small case each ------------------------------------------------------------------------------------
def check_pool(lib, n_new=5):
    """pooled generate() calls of two sessions in flight together give the ids of the lone session loop"""
    import threading

    eng = make_engine("ds_img_depth_seg", lib)[0]
    cases = [e2e_cases.fixture_inputs(n)[2:] for n in ("ds_img_depth_seg", "ds_img_only")]
    refs = []
    for c in cases:
        last, _, _ = eng.prefill(*c, reserve=n_new)
        toks = [np.argmax(last, -1).astype(np.int32)]
        for _ in range(n_new - 1):
            toks.append(eng.decode_step(toks[-1], want_logits=False)[1])
        refs.append(np.stack(toks, 1))
    sessions, outs, errs = [eng, eng.fork()], [None, None], []

    def work(i):
        try:
            outs[i] = [sessions[i].generate_greedy(*cases[(i + j) % 2], max_new_tokens=n_new) for j in range(2)]
        except BaseException as e:
            errs.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    for i in range(2):
        for j in range(2):
            assert np.array_equal(outs[i][j], refs[(i + j) % 2]), f"session {i} request {j}: pooled ids differ from the session loop"
    sessions[1].close()
    eng.close()


def tiny_checkpoint(dirpath):
    """a tiny vcoder_ds checkpoint in HF layout under dirpath -> (directory, model name)"""
    import os

    from vcoder_amd import checkpoint, config as vcfg

    name = "vcoder_ds_llava-tiny"
    d = os.path.join(str(dirpath), name)
    cfg = vcfg.tiny("vcoder_ds")
    checkpoint.save_checkpoint(d, cfg.to_hf_dict(), synth.synth_state_dict(cfg, 42), bf16=True)
    return d, name


def load_model(d, name, lib=None):
    """lib None: load_pretrained_model(d, None, name, weight_format="w4a16") on the product library; else the layer right below it
    (from_tensors) on that library — the emulator"""
    if lib is None:
        from vcoder_amd.model.builder import load_pretrained_model

        return load_pretrained_model(d, None, name, weight_format="w4a16")[1]
    from vcoder_amd import checkpoint, config as vcfg
    from vcoder_amd.model import language_model as lm

    cfg = vcfg.VCoderConfig.from_pretrained(d, name)
    return lm.VCoderDSLlavaLlamaForCausalLM.from_tensors(cfg, checkpoint.iter_checkpoint_tensors(d), weight_format="w4a16", _lib_override=lib)


def check_model_ids(model, lib=None, n_new=4):
    """the loaded model generates the ids of an engine told set_weight_format("w4a16") on the same weights"""
    assert model.engine.weight_format == "w4a16"
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs("ds_img_depth_seg")
    assert int(g["seed"]) == 42
    t = torch.from_numpy
    out = model.generate(t(ids), images=t(imgs), segs=t(segs), depths=t(deps), do_sample=False, max_new_tokens=n_new, eos_token_id=-1)
    eng = make_engine("ds_img_depth_seg", lib)[0]
    want = eng.generate_greedy(ids, imgs, segs, deps, max_new_tokens=n_new)
    eng.close()
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), want), (out[:, ids.shape[1]:].tolist(), want.tolist())


def check_beams(model):
    """generate(num_beams=2): the device loop equals the host loop (beam_cases.check_engine_case, which asserts the case's margin)"""
    import beam_cases as bc

    return bc.check_engine_case(model, "bf16", "mm", 2, 2, 5, 0)
