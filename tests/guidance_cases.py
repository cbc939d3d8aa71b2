"""Classifier-free guidance inside the device decode loop (vck_guidance_combine, vck_guidance_follow, vc_request_guidance,
generate(guidance_scale=, negative_prompt_ids=, negative_images= ...)): the checks shared by the CPU-emulator tests
(tests/test_guidance_emu.py) and the `-m gpu` tests (tests/test_gpu_guidance.py).

The definition, for a raw conditional row c, a raw unconditional row u of the same step and a scale g (fp32):
    lc = (c - max c) - log(sum exp(c - max c)),   lu likewise,   out = g * (lc - lu) + lu      (product and sum rounded separately)
The combine kernel leaves its four reduction scalars per pair, so `ref_combine` — numpy float32 — must reproduce `out` bit for bit;
the scalars themselves are held against float64 at score_cases.KERNEL_BAR, the bar the log-prob kernels' tests apply to the same
quantity (a row's max + log sum exp)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import e2e_cases
import kernel_cases as kc
import logits_processor_cases as pc
import logprob_cases as lc
from score_cases import KERNEL_BAR
from vcoder_amd import logits_processors as lp

RS_GD_SCALE = 113   # csrc/kernels.h RowStateField
SCALES = (0.5, 1.5, 3.0)

# ---- the combine kernel ------------------------------------------------------------------------------------------------------
# (pairs, V, ldl, ldo, floats the raw rows' base is shifted by, floats `out` is shifted by, layout).  layout "pair": the conditional
# and the unconditional rows in two buffers with the same shift (row r of both starts at the same offset modulo 16 bytes); "stacked":
# one buffer of 2 B rows, the unconditional rows B * ldl floats behind the conditional ones — the engine's layout.
# V = 37: tails only, most threads idle; V = 4099: the 16-byte body takes some threads twice (1024 threads x 4 floats) and leaves a
# scalar tail; ldl = V + 1 with shifts 1, 2, 3: every misalignment of a row start; ldo != ldl: `out` rows that are not congruent
# with their sources (pass 2 goes scalar) and pad columns of their own.
COMBINE_SHAPES_EMU = [
    (1, 37, 37, 37, 0, 0, "pair"), (2, 37, 38, 40, 1, 1, "pair"), (3, 37, 38, 38, 2, 2, "stacked"), (1, 37, 38, 41, 3, 0, "stacked"),
    (3, 4099, 4100, 4100, 0, 0, "pair"), (2, 4099, 4100, 4104, 1, 1, "pair"), (2, 4099, 4100, 4101, 2, 3, "pair"),
    (2, 4099, 4100, 4100, 3, 3, "stacked"), (2, 320, 320, 320, 0, 0, "stacked"),
]
COMBINE_SHAPES_GPU = COMBINE_SHAPES_EMU + [
    (1, 32000, 32000, 32000, 0, 0, "stacked"), (8, 32000, 32000, 32000, 0, 0, "stacked"), (2, 32000, 32001, 32004, 1, 1, "pair"),
    (2, 32000, 32001, 32001, 2, 2, "pair"), (2, 32000, 32001, 32003, 3, 1, "pair"),
]
COMBINE_KINDS = ["random", "reach80", "identical", "offset", "peaked"]


def _pair(kind, V, rng):
    """-> (c, u) fp32 rows, finite"""
    c = (rng.randn(V) * 3).astype(np.float32)
    u = (rng.randn(V) * 3).astype(np.float32)
    if kind == "reach80":   # values up to +-80: exp() of the raw values would overflow / vanish, the max subtraction matters
        c = (c * np.float32(8)).astype(np.float32)
        u = (u * np.float32(8)).astype(np.float32)
        c[rng.randint(0, V)] = np.float32(80.0)
        c[rng.randint(0, V)] = np.float32(-80.0)
        u[rng.randint(0, V)] = np.float32(-80.0)
        u[:] = u - np.float32(70.0)
        u[rng.randint(0, V)] = np.float32(80.0)
    elif kind == "identical":
        u = c.copy()
    elif kind == "offset":   # the same distribution: lu == lc up to rounding
        u = (c + np.float32(5.0)).astype(np.float32)
    elif kind == "peaked":
        c[rng.randint(0, V)] = np.float32(40.0)
    return c, u


def ref_combine(c, u, scalars, g):
    """numpy float32 restatement of the kernel's second pass from its own four scalars"""
    mc, lsc, mu, lsu = (np.float32(s) for s in scalars)
    lcv = (c - mc) - lsc
    luv = (u - mu) - lsu
    return (np.float32(g) * (lcv - luv) + luv).astype(np.float32), lcv.astype(np.float32)


def check_guidance_combine(be, B, V, ldl, ldo, shift, oshift, layout, seed=0):
    """launches of B pairs each until every kind of pair has run; NaN in the pad columns of the raw rows, in front of the first and
    behind the last row (an element read too many poisons the scalars); a sentinel in every float of `out` and `scalars` that must
    stay.  The last launch has an inactive pair when B > 1.
    -> the largest deviation of max + log sum from float64 logsumexp"""
    assert all(a.dtype == np.float32 for a in _pair("random", 8, np.random.RandomState(0)))
    rng = np.random.RandomState(seed + B * 7 + V)
    worst = 0.0
    n_launch = -(-len(COMBINE_KINDS) // B)
    SENT = np.float32(-12345.5)
    for launch in range(n_launch):
        kinds = [COMBINE_KINDS[(launch * B + r) % len(COMBINE_KINDS)] for r in range(B)]
        scales = [SCALES[(launch + r) % len(SCALES)] for r in range(B)]
        pairs = [_pair(k, V, rng) for k in kinds]
        if layout == "stacked":
            raw = np.full(shift + 2 * B * ldl + 3, np.nan, dtype=np.float32)
            for r, (c, u) in enumerate(pairs):
                raw[shift + r * ldl: shift + r * ldl + V] = c
                raw[shift + (B + r) * ldl: shift + (B + r) * ldl + V] = u
            d_raw = be.f32(raw)
            d_c, d_u, keep = d_raw[shift:], d_raw[shift + B * ldl:], [(d_raw, raw)]
        else:
            rc = np.full(shift + B * ldl + 3, np.nan, dtype=np.float32)
            ru = rc.copy()
            for r, (c, u) in enumerate(pairs):
                rc[shift + r * ldl: shift + r * ldl + V] = c
                ru[shift + r * ldl: shift + r * ldl + V] = u
            d_rc, d_ru = be.f32(rc), be.f32(ru)
            d_c, d_u, keep = d_rc[shift:], d_ru[shift:], [(d_rc, rc), (d_ru, ru)]
        rec = kc.make_rows(B)
        for r in range(B):
            rec[r, RS_GD_SCALE] = kc._f32_bits(scales[r])
        off = B - 1 if (launch == n_launch - 1 and B > 1) else -1   # the inactive pair
        if off >= 0:
            rec[off, kc.RS["ACTIVE"]] = 0
        d_rec = be.i32(rec)
        d_out = be.f32(np.full(oshift + B * ldo + 3, SENT, dtype=np.float32))
        d_sc = be.f32(np.full((B + 1) * 4, SENT, dtype=np.float32))
        kc._call(be, "vck_guidance_combine", d_c, d_u, ldl, d_out[oshift:], ldo, d_rec, d_sc, B, V)
        got, sc = be.host_f32(d_out), be.host_f32(d_sc)
        for d, h in keep:
            assert np.array_equal(be.host_f32(d).view(np.int32), h.view(np.int32)), "a raw row was written"
        assert np.array_equal(be.host_i32(d_rec), rec), "the records were written"
        assert (got[:oshift] == SENT).all() and (got[oshift + B * ldo:] == SENT).all(), "wrote in front of the first / behind the last row"
        assert (sc[B * 4:] == SENT).all(), "wrote behind the last pair's scalars"
        for r, (c, u) in enumerate(pairs):
            what = f"guidance_combine B {B} V {V} ldl {ldl} ldo {ldo} shift {shift}/{oshift} {layout} launch {launch} row {r} ({kinds[r]}, g {scales[r]})"
            row = got[oshift + r * ldo: oshift + (r + 1) * ldo]
            assert (row[V:] == SENT).all(), f"{what}: pad columns written"
            s = sc[r * 4: r * 4 + 4]
            if r == off:
                assert (row == SENT).all() and (s == SENT).all(), f"{what}: an inactive pair was written"
                continue
            # 2. the scalars against float64
            assert s[0] == c.max() and s[2] == u.max(), f"{what}: maxima {s[0]}, {s[2]} vs {c.max()}, {u.max()}"
            for (m, ls), v in (((s[0], s[1]), c), ((s[2], s[3]), u)):
                dev = abs((float(m) + float(ls)) - float(np.logaddexp.reduce(v.astype(np.float64))))
                worst = max(worst, dev)
                assert dev < KERNEL_BAR, f"{what}: max + log sum deviates from float64 logsumexp by {dev}"
            # 1. bit for bit from the kernel's own scalars
            ref, lcv = ref_combine(c, u, s, scales[r])
            assert np.isfinite(ref).all()
            bad = np.nonzero(row[:V].view(np.int32) != ref.view(np.int32))[0]
            assert bad.size == 0, f"{what}: ids {bad[:8]}: got {row[bad[:8]]}, restatement {ref[bad[:8]]}"
            if kinds[r] == "identical":
                assert np.array_equal(s[:2].view(np.int32), s[2:].view(np.int32)), f"{what}: identical rows reduce differently"
                assert np.array_equal(row[:V].view(np.int32), lcv.view(np.int32)), f"{what}: identical rows: out is not lc"
            # the formula in float64, to fp32 rounding of its three log-domain terms (|lc|, |lu| and g |lc - lu| each below 2^9 here)
            c64, u64 = c.astype(np.float64), u.astype(np.float64)
            l64c, l64u = c64 - np.logaddexp.reduce(c64), u64 - np.logaddexp.reduce(u64)
            want = scales[r] * (l64c - l64u) + l64u
            tol = (4 + 2 * scales[r]) * (np.abs(l64c).max() + np.abs(l64u).max()) * 2.0 ** -23 + (1 + 2 * scales[r]) * KERNEL_BAR
            assert np.abs(row[:V] - want).max() < tol, f"{what}: deviates from the float64 formula by {np.abs(row[:V] - want).max()} (bar {tol})"
    print(f"guidance_combine B {B} V {V} {layout}: scalars within {worst:.2e} of float64 (bar {KERNEL_BAR:.1e})")
    return worst


# ---- the follow kernel -------------------------------------------------------------------------------------------------------
FOLLOW_SHAPES_EMU = [(1, 64, 16, 3), (3, 136, 16, 3), (2, 64, 16, 1)]   # (B, D, npart, advance)
FOLLOW_SHAPES_GPU = FOLLOW_SHAPES_EMU + [(8, 4096, 256, 3), (2, 5120, 320, 3)]


def check_guidance_follow(be, B, D, npart, advance, seed=0):
    """rows 0 .. B - 1 hold what a selection left, rows B .. 2 B - 1 follow; two more rows behind them and every buffer's tail must stay.
    Different start positions per row; the partners' RS_FINISHED mixed; with B > 1 the last follower is inactive."""
    rng = np.random.RandomState(seed + B * 11 + D)
    R = 2 * B + 2
    rec = kc.make_rows(R)
    rec[:, kc.RS["POS"]] = 100 + 7 * np.arange(R)
    rec[:, kc.RS["STEP"]] = 3 + np.arange(R)
    rec[:B, kc.RS["FINISHED"]] = np.arange(B) % 2 == 0
    rec[B: 2 * B, kc.RS["FINISHED"]] = np.arange(B) % 2 == 1   # what a follower held is replaced
    rec[B: 2 * B, kc.RS["MAXNEW"]] = 0
    off = 2 * B - 1 if B > 1 else -1
    if off >= 0:
        rec[off, kc.RS["ACTIVE"]] = 0
    tok = rng.randint(0, 32000, size=R).astype(np.int32)
    x = rng.randn(R, D).astype(np.float32)
    ssq = rng.rand(R, npart).astype(np.float32)
    xg = rng.randint(0, 65536, size=(R, D)).astype(np.uint16)
    d_rec, d_tok, d_x, d_ssq, d_xg = be.i32(rec), be.i32(tok), be.f32(x), be.f32(ssq), be.bits16(xg)
    kc._call(be, "vck_guidance_follow", d_rec, d_tok, d_x, d_ssq, d_xg, B, D, npart, advance)
    g_rec, g_tok, g_x, g_ssq = be.host_i32(d_rec), be.host_i32(d_tok), be.host_f32(d_x), be.host_f32(d_ssq)
    g_xg = kc.raw_bits(d_xg).reshape(R, D)
    w_rec, w_tok, w_x, w_ssq, w_xg = rec.copy(), tok.copy(), x.copy(), ssq.copy(), xg.copy()
    for i in range(B):
        f = B + i
        if f == off:
            continue
        w_tok[f], w_x[f], w_ssq[f], w_xg[f] = tok[i], x[i], ssq[i], xg[i]
        w_rec[f, kc.RS["FINISHED"]] = rec[i, kc.RS["FINISHED"]]
        w_rec[f, kc.RS["STEP"]] += advance & 1
        w_rec[f, kc.RS["POS"]] += (advance >> 1) & 1
    what = f"guidance_follow B {B} D {D} npart {npart} advance {advance}"
    assert np.array_equal(g_tok, w_tok), f"{what}: next_tok {g_tok} vs {w_tok}"
    assert np.array_equal(g_x.view(np.int32), w_x.view(np.int32)), f"{what}: x rows"
    assert np.array_equal(g_ssq.view(np.int32), w_ssq.view(np.int32)), f"{what}: sum-of-squares partials"
    assert np.array_equal(g_xg, w_xg), f"{what}: xg rows"
    assert np.array_equal(g_rec, w_rec), f"{what}: records differ in rows {np.nonzero((g_rec != w_rec).any(1))[0]}"


# ---- the torch restatement (logits_processors.apply_guidance) ------------------------------------------------------------------
def check_restatement():
    """apply_guidance against the formula in float64, to fp32 rounding"""
    rng = np.random.RandomState(5)
    for V, g in ((37, 0.5), (4099, 1.5), (32000, 3.0)):
        c = torch.from_numpy((rng.randn(3, V) * 4).astype(np.float32))
        u = torch.from_numpy((rng.randn(3, V) * 4).astype(np.float32))
        got = lp.apply_guidance(c, u, g)
        assert got.dtype == torch.float32 and got.shape == c.shape
        l64c, l64u = torch.log_softmax(c.double(), -1), torch.log_softmax(u.double(), -1)
        want = g * (l64c - l64u) + l64u
        tol = (4 + 2 * g) * float(l64c.abs().max() + l64u.abs().max()) * 2.0 ** -23 + (1 + 2 * g) * KERNEL_BAR
        assert float((got.double() - want).abs().max()) < tol
        same = lp.apply_guidance(c, c.clone(), g)
        assert float((same.double() - l64c).abs().max()) < tol


def check_restatement_against_hf():
    """apply_guidance against Transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor driven by a stub model that returns the
    unconditional logits.  -> False when the installed Transformers has no such class (the caller skips)"""
    rng = np.random.RandomState(6)
    try:
        from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as HF
    except Exception:
        return False

    V, g = 101, 1.5
    c = torch.from_numpy((rng.randn(2, V) * 4).astype(np.float32))
    u = torch.from_numpy((rng.randn(2, V) * 4).astype(np.float32))

    class Out(dict):   # a ModelOutput is read both ways: out.get("past_key_values") and out.logits
        def __init__(self, logits):
            super().__init__(logits=logits, past_key_values=None)
            self.logits = logits

    class Stub:   # returns the unconditional logits as the last position, whatever it is fed
        def __call__(self, input_ids, **kw):
            return Out(u[:, None, :].expand(-1, input_ids.shape[1], -1).contiguous())

    ids = torch.zeros(2, 4, dtype=torch.long)
    proc = HF(g, Stub(), unconditional_ids=ids, use_cache=False)
    want = proc(ids, c.clone())
    got = lp.apply_guidance(c, u, g)
    assert float((got - want).abs().max()) < (4 + 2 * g) * float(want.abs().max()) * 2.0 ** -23 + (1 + 2 * g) * KERNEL_BAR
    return True


# ---- engine and model ------------------------------------------------------------------------------------------------------------
N_NEW = 6
SCALE = 1.5
_models = {}


def model_for(variant, lib=None, operands="bf16", fmt="bf16", seed=42):
    """one model per (variant, library, weight format) for the tests of this feature alone, released by close_models() when a module
    is through (as constraint_cases.model_for: the sessions other modules share keep their buffers and captured steps)"""
    import score_cases as sc

    key = (variant, id(lib), operands, fmt)
    if key not in _models:
        kw = {"_lib_override": lib} if lib is not None else {}
        m = sc._CLASSES[variant](e2e_cases.tiny_cfg(variant), device="cuda", operands=operands, **kw)
        m.engine.load_synthetic(seed)
        if fmt != "bf16":
            m.engine.set_weight_format(fmt)
        m.finalize_weights()
        _models[key] = m
    return _models[key]


def close_models():
    for m in _models.values():
        m.engine.close()
    _models.clear()


FIXTURE = {"vcoder_ds": "ds_img_depth_seg", "vcoder": "vc_img_seg"}


def inputs_for(variant, B):
    """the multimodal prompts of the variant's fixture (B = 2; B = 1: its first row) -> (ids [B, T] int64, pixel kwargs)"""
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(FIXTURE[variant])
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[:B]))
    return ids[:B].copy(), dict(images=t(imgs), segs=t(segs), depths=t(deps))


def negatives_for(variant, ids, px):
    """the three kinds of negative prompt: HF's default (none given), the question without its pictures (text-only,
    mm_utils.strip_placeholders), the same ids with blanked seg / depth maps"""
    from vcoder_amd import mm_utils

    blank = lambda a: None if a is None else torch.zeros_like(a)
    return {
        "default": {},
        "text": dict(negative_prompt_ids=mm_utils.strip_placeholders(torch.from_numpy(ids))),
        "pixels": dict(negative_prompt_ids=torch.from_numpy(ids), negative_images=px["images"], negative_segs=blank(px["segs"]),
                       negative_depths=blank(px["depths"])),
    }


def _gen(model, ids, px, **kw):
    kw.setdefault("max_new_tokens", N_NEW)
    kw.setdefault("eos_token_id", -1)
    return model.generate(torch.from_numpy(ids), **px, **kw)


def _both(model, ids, px, what, **kw):
    """the guided call on the device loop and on the host loop: the same tensor, and the engine reports the request as served"""
    B = ids.shape[0]
    dev = _gen(model, ids, px, guidance_scale=SCALE, **kw)
    lg = model.engine.last_guidance
    n = int(kw.get("num_return_sequences", 1))
    assert lg is not None and lg["rows"] == 2 * B * n, f"{what}: last_guidance {lg}"
    host = _gen(model, ids, px, guidance_scale=SCALE, processors_on_device=False, **kw)
    assert model.engine._cur_batch == 2 * B * n, f"{what}: processors_on_device=False did not take the host loop over 2 B rows"
    d, h = (dev.sequences, host.sequences) if hasattr(dev, "sequences") else (dev, host)
    T = ids.shape[1]
    assert torch.equal(d, h), f"{what}: device loop {d[:, T:].tolist()}, host loop {h[:, T:].tolist()}"
    return dev, host


def check_device_vs_host(model, variant, B):
    """5: greedy and sampled (top_k = 1: the one candidate both samplers must pick, as constraint_cases) guided calls with every
    kind of negative prompt: device loop == host loop; the text-only negative prompt changes the plain call's ids"""
    ids, px = inputs_for(variant, B)
    T = ids.shape[1]
    plain = _gen(model, ids, px)
    for name, nkw in negatives_for(variant, ids, px).items():
        dev, _ = _both(model, ids, px, f"{variant} B {B} {name} greedy", **nkw)
        print(f"{variant} B {B} negative {name}: plain {plain[:, T:].tolist()} guided {dev[:, T:].tolist()} {model.engine.last_guidance}")
        if name == "text":
            assert not torch.equal(dev, plain), f"{variant} B {B}: guidance changes nothing: the case shows nothing"
            neg_T = int(nkw["negative_prompt_ids"].shape[1])
            assert model.engine.last_guidance["negative_len"] == neg_T and model.engine.last_guidance["prompt_len"] > T
        skw = dict(do_sample=True, temperature=0.9, top_k=1, top_p=0.95, seed=11)
        _both(model, ids, px, f"{variant} B {B} {name} sampled", **nkw, **skw)
    # the usual sampler settings: the guided sampled call repeats under its seed and differs from the unguided one's stream
    skw = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=11)
    nkw = negatives_for(variant, ids, px)["text"]
    a = _gen(model, ids, px, guidance_scale=SCALE, **nkw, **skw)
    assert torch.equal(a, _gen(model, ids, px, guidance_scale=SCALE, **nkw, **skw)), "a sampled guided call does not repeat under its seed"


def check_sampled_support(model, variant, B=2, seeds=(11, 12, 13)):
    """the device's Gumbel-max over the guided rows against an independent reference: every id a sampled guided call (temperature 0.9,
    top_k 30, top_p 0.95) emits must lie in the support of the host's warped distribution of that step's guided scores — the 2 B raw
    rows of the host loop's primitives, teacher-forced with the device's ids, through the torch formula and HF's warper order.  An
    id at the edge of the kept set may flip with the rounding of the scores: the slack is the (4 g + 2) KERNEL_BAR of check_restatement."""
    from vcoder_amd.model import language_model as lm

    eng = model.engine
    ids, px = inputs_for(variant, B)
    T = ids.shape[1]
    neg = negatives_for(variant, ids, px)["text"]["negative_prompt_ids"]
    temp, top_k, top_p = 0.9, 30, 0.95
    seen = set()
    for seed in seeds:
        new = _gen(model, ids, px, guidance_scale=SCALE, negative_prompt_ids=neg, do_sample=True, temperature=temp, top_k=top_k,
                   top_p=top_p, seed=seed)[:, T:].numpy()
        assert eng.last_guidance is not None and eng._cur_batch == B
        last, _ = eng.prefill_guided(ids, px["images"], px["segs"], px["depths"], guidance=lp.Guidance(SCALE, neg.numpy()), reserve=N_NEW)
        eng.clear_attention_mask()
        lg = torch.from_numpy(last)
        for s_ in range(new.shape[1]):
            sc = (SCALE * (torch.log_softmax(lg[:B].float(), -1) - torch.log_softmax(lg[B:].float(), -1)) + torch.log_softmax(lg[B:].float(), -1)) / temp
            kth = torch.topk(sc, top_k)[0][..., -1, None]
            kept = lm._top_p_filter(sc.masked_fill(sc < kth, float("-inf")), top_p)
            for b in range(B):
                t_, floor = int(new[b, s_]), float(kept[b][torch.isfinite(kept[b])].min())
                assert float(sc[b, t_]) >= floor - (4 * SCALE + 2) * KERNEL_BAR / temp, \
                    f"seed {seed} row {b} step {s_}: id {t_} (score {float(sc[b, t_]):.4f}) lies outside the warped support (floor {floor:.4f})"
                seen.add((b, s_, t_))
            if s_ + 1 < new.shape[1]:
                tok = np.ascontiguousarray(new[:, s_], dtype=np.int32)
                lg = torch.from_numpy(eng.decode_step(np.concatenate([tok, tok]))[0])
    assert len(seen) > B * N_NEW, "every seed drew the same ids: the sampler is not exercised"


def check_with_everything(model, variant, B=2):
    """5: the guided call with all five processors, with a TokenAutomaton, with log-probs, with EOS ids that fire at different steps
    per row, with a streamer, with num_return_sequences = 2: device loop == host loop"""
    from vcoder_amd.constraints import TokenAutomaton

    eng = model.engine
    ids, px = inputs_for(variant, B)
    T, V = ids.shape[1], model.config.vocab_size
    nkw = negatives_for(variant, ids, px)["text"]
    guided = _gen(model, ids, px, guidance_scale=SCALE, **nkw)
    new = guided[:, T:].numpy()
    # -- the five processors (history: input_ids + generated ids; the penalty reads the guided, log-domain rows)
    pkw = pc.configs_from(guided, T)["all_five"][0]
    dev, _ = _both(model, ids, px, f"{variant} processors", **nkw, **pkw)
    assert not torch.equal(dev, guided) or dev.shape != guided.shape, "the processors change nothing behind guidance"
    pen, _ = _both(model, ids, px, f"{variant} repetition penalty", **nkw, repetition_penalty=pc.REP_PENALTY)
    # -- a token automaton over ids the guided call never emits
    used = {int(t) for t in new.reshape(-1)}
    A = [t for t in range(7, V) if t not in used][:: max((V - 7 - len(used)) // 8, 1)][:8]
    a = TokenAutomaton.from_sequences([[A[0], A[1], A[2]], [A[0], A[3]], [A[4], A[4], A[4], A[4]]], [A[5]])
    dev, _ = _both(model, ids, px, f"{variant} automaton", **nkw, constraint=a, eos_token_id=A[5], pad_token_id=0)
    for b in range(B):
        row = [int(t) for t in dev[b, T:]]
        row = row[: row.index(A[5]) + 1] if A[5] in row else row
        assert a.walk(row) != -1, f"{variant} automaton row {b}: {row} is rejected"
    # -- log-probs: those of the RAW conditional rows — step 0's are the plain call's, bit for bit — and equal ids / top ids on both loops
    lkw = dict(output_logprobs=True, top_logprobs=3)
    dev, host = _both(model, ids, px, f"{variant} log-probs", **nkw, **lkw)
    assert torch.equal(dev.sequences, guided), "the ids change with the log-prob request"
    assert torch.equal(dev.top_token_ids, host.top_token_ids)
    assert float((dev.token_logprobs - host.token_logprobs).abs().max()) < 2 * KERNEL_BAR
    assert float((dev.top_logprobs - host.top_logprobs).abs().max()) < 2 * KERNEL_BAR
    base = _gen(model, ids, px, **lkw)
    assert np.array_equal(dev.top_logprobs[:, 0].numpy().view(np.int32), base.top_logprobs[:, 0].numpy().view(np.int32)) and \
        torch.equal(dev.top_token_ids[:, 0], base.top_token_ids[:, 0]), "step 0: not the log-probs of the raw conditional row"
    # -- EOS ids that fire at different steps per row (the second becomes a stop sequence on the device)
    # (under HF's default negative prompt, whose rows vary more than those of the text-only one on this model)
    nkw_text, nkw = nkw, {}
    new = _gen(model, ids, px, guidance_scale=SCALE)[:, T:].numpy()
    e0 = int(new[0, 1])
    e1 = next((int(t) for t in new[1, 3:] if int(t) != e0 and int(t) not in new[0].tolist()), None)
    assert e1 is not None, f"no second EOS id in row 1 of {new.tolist()}: the case shows nothing"
    eos = [e0, e1]
    dev, _ = _both(model, ids, px, f"{variant} EOS {eos}", **nkw, eos_token_id=eos, pad_token_id=0)
    got = dev[:, T:].numpy()
    assert pc.finish_end(got[0], set(eos)) == pc.finish_end(new[0], set(eos)) and (got[0, pc.finish_end(got[0], set(eos)):] == 0).all()
    assert np.array_equal(got[1, : pc.finish_end(got[1], set(eos))], new[1, : pc.finish_end(new[1], set(eos))])
    # -- an EOS id (row 0, step 1) beside a 2-token stop sequence on the device (row 1: a criterion with device_stop_sequences)
    class Stop:
        def __init__(self, seq):
            self.seq = [int(t) for t in seq]

        def device_stop_sequences(self):
            return [self.seq]

    pair = next(([int(new[1, j]), int(new[1, j + 1])] for j in range(1, N_NEW - 2)
                 if e0 not in new[1, : j + 2].tolist()
                 and not any(new[1, i: i + 2].tolist() == new[1, j: j + 2].tolist() for i in range(j))
                 and not any(new[0, i: i + 2].tolist() == new[1, j: j + 2].tolist() for i in range(1))), None)
    assert pair is not None, f"no 2-token stop sequence in row 1 of {new.tolist()}: the case shows nothing"
    j = next(i for i in range(N_NEW - 1) if new[1, i: i + 2].tolist() == pair)
    out = _gen(model, ids, px, guidance_scale=SCALE, stopping_criteria=[Stop(pair)], eos_token_id=e0, pad_token_id=0, **nkw)[:, T:].numpy()
    assert eng.last_guidance is not None and eng._cur_batch == B, "a device stop sequence beside guidance left the device loop"
    f0 = pc.finish_end(new[0], {e0})
    assert f0 != j + 2, "the two rows finish at the same step: the case shows nothing"
    assert out[0].tolist() == (new[0, :f0].tolist() + [0] * N_NEW)[: out.shape[1]], f"row 0 {out[0].tolist()}: EOS {e0} ends it at {f0}, then pad"
    assert out.shape[1] == max(j + 2, f0) and out[1].tolist() == (new[1, : j + 2].tolist() + [0] * N_NEW)[: out.shape[1]], \
        f"row 1 {out[1].tolist()}: stops behind {pair} at step {j + 1}"
    nkw, new = nkw_text, guided[:, T:].numpy()
    # -- a streamer receives the returned ids, B rows wide
    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got.append(v.clone())

        def end(self):
            pass

    for on_device in (True, False):
        s = Streamer()
        out = _gen(model, ids, px, guidance_scale=SCALE, streamer=s, processors_on_device=on_device, **nkw)
        assert torch.equal(out, guided)
        assert torch.equal(s.got[0], torch.from_numpy(ids))
        assert torch.equal(torch.stack([p.reshape(-1) for p in s.got[1:]], 1), out[:, T:]), "the streamed pieces are not the returned ids"
    # -- num_return_sequences = 2: rows b n + j; the call on the repeated inputs with the same seed
    skw = dict(do_sample=True, temperature=0.9, top_k=1, top_p=0.95, seed=11, num_return_sequences=2)
    dev, _ = _both(model, ids, px, f"{variant} num_return_sequences", **nkw, **skw)
    assert dev.shape[0] == 2 * B
    skw = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=11)
    two = _gen(model, ids, px, guidance_scale=SCALE, num_return_sequences=2, fan_out=True, **nkw, **skw)
    rep = np.repeat(np.arange(B), 2)
    rpx = {k: (None if v is None else v[rep]) for k, v in px.items()}
    want = _gen(model, ids[rep], rpx, guidance_scale=SCALE, negative_prompt_ids=nkw["negative_prompt_ids"][rep], **skw)
    assert torch.equal(two, want), "num_return_sequences = 2 is not the call on the repeated inputs"
    assert eng.last_fanout is None


def check_oracle_anchor(lib=None, variant="vcoder_ds", n_new=N_NEW, modes=("strict", "split")):
    """6: greedy guided ids against two FREE-RUNNING streams of the fp32 oracle (oracle/cpu_ref.py) — behind the prompt and behind
    the text-only negative prompt, each fed the oracle's own choice — combined by the formula in torch.  In the precision modes whose
    end-to-end tests assert the ids bit-exact with no margin (e2e_cases.check_fixture_strict: "strict" and "split"), with that rule:
    plain array_equal.  The device's guided scores of every step (its 2 B raw rows through the same torch formula) are held against
    the oracle's as well: each raw row within e2e_cases.TOL_STRICT of the oracle's, the bar of those tests, and so the guided scores
    within (4 g + 2) TOL_STRICT (two log-softmaxes of rows that are TOL_STRICT off move by at most 2 TOL_STRICT each)."""
    import cpu_ref
    from vcoder_amd import mm_utils, synth

    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(FIXTURE[variant])
    model = model_for(variant, lib)
    eng = model.engine
    t = lambda a: None if a is None else torch.from_numpy(a)
    px = dict(images=t(imgs), segs=t(segs), depths=t(deps))
    neg = mm_utils.strip_placeholders(ids)
    B, T = ids.shape
    formula = lambda c, u: SCALE * (torch.log_softmax(c.float(), -1) - torch.log_softmax(u.float(), -1)) + torch.log_softmax(u.float(), -1)
    om = cpu_ref.OracleModel(cfg, synth.synth_state_dict(cfg, int(g["seed"])), emu_bf16=False)
    with torch.no_grad():
        oc, cache_c = om.forward(ids.tolist(), px["images"], px["segs"], px["depths"], last_only=True)
        ou, cache_u = om.forward(neg.tolist(), None, last_only=True)
        want, raws = [], []
        for s_ in range(n_new):
            raws.append((oc[:, -1].float().clone(), ou[:, -1].float().clone()))
            nxt = torch.argmax(formula(*raws[-1]), -1)
            want.append(nxt)
            if s_ + 1 < n_new:
                oc, ou = om.decode_step(nxt.tolist(), cache_c), om.decode_step(nxt.tolist(), cache_u)
    want = torch.stack(want, 1).numpy()
    plain = om.generate_greedy(ids.tolist(), px["images"], px["segs"], px["depths"], max_new_tokens=n_new).numpy()
    assert not np.array_equal(want, plain), "the oracle's guided ids are its plain ids: the anchor shows nothing"
    for mode in modes:
        eng.set_precision(mode)
        try:
            got = _gen(model, ids, px, guidance_scale=SCALE, negative_prompt_ids=torch.from_numpy(neg), max_new_tokens=n_new)[:, T:].numpy()
            assert eng.last_guidance is not None and eng.last_guidance["rows"] == 2 * B
            print(f"oracle anchor {variant} [{mode}]: ids {got.tolist()}, oracle {want.tolist()}")
            assert np.array_equal(got, want), f"[{mode}] guided ids {got.tolist()} differ from the oracle's {want.tolist()}"
            # the raw rows and the guided scores of every step, teacher-forced with those ids
            last, _ = eng.prefill_guided(ids, px["images"], px["segs"], px["depths"], guidance=lp.Guidance(SCALE, neg), reserve=n_new)
            eng.clear_attention_mask()
            lg = torch.from_numpy(last)
            for s_ in range(n_new):
                e_raw = max(float((lg[:B] - raws[s_][0]).abs().max()), float((lg[B:] - raws[s_][1]).abs().max()))
                assert e_raw < e2e_cases.TOL_STRICT, f"[{mode}] step {s_}: raw rows deviate from the oracle's by {e_raw}"
                e_g = float((formula(lg[:B], lg[B:]) - formula(*raws[s_])).abs().max())
                assert e_g < (4 * SCALE + 2) * e2e_cases.TOL_STRICT, f"[{mode}] step {s_}: guided scores deviate by {e_g}"
                if s_ + 1 < n_new:
                    tok = np.ascontiguousarray(want[:, s_], dtype=np.int32)
                    lg = torch.from_numpy(eng.decode_step(np.concatenate([tok, tok]))[0])
        finally:
            eng.set_precision("bf16")


def check_surface(model, variant="vcoder_ds", B=2):
    """7: None / 1.0 are no request (the plain tensor, the decode pool's steps as a plain call); the guided ids differ; the
    refusals come before the engine is touched; speculation beside guidance is not served; decode_step behind a served call refuses"""
    eng = model.engine
    ids, px = inputs_for(variant, B)
    T = ids.shape[1]
    nkw = negatives_for(variant, ids, px)["text"]
    c0 = eng.pool_step_counts()
    plain = _gen(model, ids, px)
    used = [a - b for a, b in zip(eng.pool_step_counts(), c0)]
    for g_ in (None, 1.0):
        c1 = eng.pool_step_counts()
        out = _gen(model, ids, px, guidance_scale=g_, **nkw)
        assert torch.equal(out, plain) and eng.last_guidance is None, f"guidance_scale={g_} is a request"
        assert [a - b for a, b in zip(eng.pool_step_counts(), c1)] == used, f"guidance_scale={g_} leaves the plain call's path"
    c1 = eng.pool_step_counts()
    guided = _gen(model, ids, px, guidance_scale=SCALE, **nkw)
    assert not torch.equal(guided, plain), "guidance_scale is swallowed: the guided ids are the plain call's"
    assert eng.pool_step_counts() == c1, "a guided call stepped the decode pool"
    # decode_step / extend behind a served call refuse until the next prefill
    for fn in (lambda: eng.decode_step(np.zeros(B, np.int32)), lambda: eng.extend(np.zeros((B, 2), np.int32))):
        try:
            fn()
            raise AssertionError("the session's loop is open behind a guided generate")
        except RuntimeError as e:
            assert "guided" in str(e)
    assert torch.equal(_gen(model, ids, px), plain), "a plain call behind a guided one differs"
    # refusals, before the engine is touched (the next plain call is what it was, no request is left behind)
    seg_id = int(ids[ids < 0].min())
    bad = [
        (ValueError, dict(guidance_scale=float("nan"))), (ValueError, dict(guidance_scale=float("inf"))), (ValueError, dict(guidance_scale="2")),
        (ValueError, dict(guidance_scale=SCALE, negative_prompt_ids=torch.from_numpy(ids))),                       # placeholders, no pixels
        (ValueError, dict(guidance_scale=SCALE, negative_prompt_ids=nkw["negative_prompt_ids"][:, :0])),
        (ValueError, dict(guidance_scale=SCALE, negative_prompt_ids=nkw["negative_prompt_ids"].repeat(3, 1))),
        (ValueError, dict(guidance_scale=SCALE, negative_prompt_ids=torch.tensor([[5, seg_id]]), negative_images=None)),
        (ValueError, dict(guidance_scale=SCALE, negative_images=px["images"][:1].repeat(B + 1, 1, 1, 1), **nkw)),
        (NotImplementedError, dict(guidance_scale=SCALE, negative_prompt_attention_mask=torch.zeros_like(nkw["negative_prompt_ids"]), **nkw)),
        (NotImplementedError, dict(guidance_scale=SCALE, num_beams=2, **nkw)),
        (ValueError, dict(guidance_scale=SCALE, do_sample=True, num_return_sequences=16 // (2 * B) + 1, **nkw)),
    ]
    S0 = eng.last_S
    for exc, kw in bad:
        try:
            _gen(model, ids, px, **kw)
            raise AssertionError(f"generate({list(kw)}) was accepted")
        except exc:
            pass
        assert eng.last_guidance is None and eng.last_S == S0
    # "split" / "strict": the host loop over 2 B rows, whatever processors_on_device says; the device form refuses (VC_ERR_STATE)
    for mode in ("strict", "split"):
        eng.set_precision(mode)
        try:
            base = _gen(model, ids, px)
            out = _gen(model, ids, px, guidance_scale=SCALE, **nkw)
            assert eng.last_guidance["rows"] == 2 * B and eng._cur_batch == 2 * B, f"[{mode}] not the host loop over 2 B rows"
            assert not torch.equal(out, base), f"[{mode}] guidance changes nothing"
            try:
                eng.generate(ids, px["images"], px["segs"], px["depths"], max_new_tokens=N_NEW,
                             guidance=lp.Guidance(SCALE, nkw["negative_prompt_ids"].numpy()))
                raise AssertionError(f"vc_generate served guidance in the {mode} mode")
            except RuntimeError as e:
                assert "bf16 precision mode" in str(e)
            assert torch.equal(_gen(model, ids, px), base), f"[{mode}] a plain call behind the guided ones differs"
        finally:
            eng.set_precision("bf16")
    assert torch.equal(_gen(model, ids, px), plain), "a refused request changed the next call"
    # [1, Tn] serves every row
    one = _gen(model, ids[:1].repeat(B, 0), {k: (None if v is None else v[:1].repeat(B, 1, 1, 1)) for k, v in px.items()},
               guidance_scale=SCALE, negative_prompt_ids=nkw["negative_prompt_ids"][:1])
    assert torch.equal(one[0], one[1]) and torch.equal(one[0], guided[0])
    # speculation beside guidance: not served, the guided ids
    out = _gen(model, ids, px, guidance_scale=SCALE, prompt_lookup_num_tokens=3, return_dict_in_generate=True, **nkw)
    assert out.speculation is None and torch.equal(out.sequences, guided)
    # through the ABI: refusals of the request itself; a request alone guides; a cancelled one does not; none outlives another entry point
    a = (ids, px["images"], px["segs"], px["depths"])
    neg = np.ascontiguousarray(nkw["negative_prompt_ids"].numpy(), dtype=np.int64)
    p = neg.ctypes.data_as(C.c_void_p)
    req = lambda scale, ptr=p, b=B, tn=neg.shape[1]: eng.lib.vc_request_guidance(eng._model, C.c_float(scale), ptr, b, tn, None, None, None, 0)
    assert req(float("nan")) == -1 and req(SCALE, b=0) == -1 and req(SCALE, b=9) == -1 and req(SCALE, tn=0) == -1
    want = guided[:, T:].numpy()
    assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a refused request changed the next call"
    assert req(SCALE) == 0
    assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), want), "a request through the ABI alone does nothing"
    assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "the request outlived its call"
    assert req(SCALE) == 0 and req(SCALE, ptr=None) == 0
    assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a cancelled request fired"
    assert req(SCALE) == 0
    try:
        eng.generate_beam(*a, num_beams=2, max_new_tokens=N_NEW)
        raise AssertionError("vc_generate_beam ran with a vc_request_guidance pending")
    except RuntimeError as e:
        assert "guidance" in str(e)
    assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a request outlived another entry point"


def check_abi_exports(lib):
    for name in ("vc_request_guidance", "vc_last_guidance", "vck_guidance_combine", "vck_guidance_follow"):
        assert hasattr(lib, name), f"{name} is not exported"


def check_true_dims(fmt, B=2, n_new=8):
    """8: 7b dims (V = 32000), 2 decoder + 3 ViT layers, synthetic weights, the image prompt (S = 1216) and its text-only negative
    prompt: the device loop returns what the host loop over prefill_guided + decode_step returns"""
    from vcoder_amd import config as vcfg, mm_utils, synth
    from vcoder_amd.engine import HipEngine

    cfg = vcfg.vicuna_7b("vcoder_ds")
    cfg.num_hidden_layers = 2
    cfg.vit_num_layers = 3
    V = cfg.vocab_size
    eng = HipEngine(cfg)
    try:
        eng.load_synthetic(21)
        if fmt != "bf16":
            eng.set_weight_format(fmt)
        eng.finalize()
        ids = np.stack([synth.synth_prompt_ids(V, "vcoder_ds", sample=b) for b in range(B)])
        px = synth.synth_batch(B, 336)
        gd = lp.Guidance(SCALE, mm_utils.strip_placeholders(ids))
        plain = eng.generate(ids, *px, max_new_tokens=n_new)
        dev = eng.generate(ids, *px, max_new_tokens=n_new, guidance=gd)
        assert eng.last_guidance == {"rows": 2 * B, "prompt_len": 1216, "negative_len": gd.negative_ids.shape[1]}, eng.last_guidance
        last, _ = eng.prefill_guided(ids, *px, guidance=gd, reserve=n_new)
        eng.clear_attention_mask()
        logits, host = torch.from_numpy(last).float(), []
        for step in range(n_new):
            nxt = torch.argmax(lp.apply_guidance(logits[:B], logits[B:], SCALE), dim=-1).numpy().astype(np.int32)
            host.append(nxt)
            if step + 1 < n_new:
                logits = torch.from_numpy(eng.decode_step(np.concatenate([nxt, nxt]))[0]).float()
        host = np.stack(host, 1)
        print(f"7b dims {fmt} B {B}: plain {plain.tolist()} guided {dev.tolist()}")
        assert np.array_equal(dev, host), f"7b dims {fmt}: device {dev.tolist()}, host loop {host.tolist()}"
        assert np.array_equal(eng.generate(ids, *px, max_new_tokens=n_new), plain), "a plain call behind the guided one differs"
    finally:
        eng.close()
