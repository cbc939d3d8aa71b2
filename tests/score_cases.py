"""Scoring target tokens on the device (vck_token_logprob, vc_request_token_scores / vc_rewind, forward(labels=), score(),
KVCacheHandle.crop): the checks shared by the CPU-emulator tests (tests/test_score_emu.py) and the `-m gpu` tests
(tests/test_gpu_score.py).  Ground truth of the label splice and the loss: tests/golden/score_cases.npz, recorded from the reference
(tools/gen_score_golden.py)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import e2e_cases
import kernel_cases as kc
from vcoder_amd import _lib, synth
from vcoder_amd.model import language_model as lm

IGNORE = -100
SCORE = np.load(os.path.join(e2e_cases.GOLD, "score_cases.npz"))
CASES = json.loads(str(SCORE["cases"]))

# ---- kernel ------------------------------------------------------------------------------------------------------------------
# Largest deviation of vck_token_logprob from numpy float64 log-softmax over the finite cases below, measured over every shape of
# KERNEL_SHAPES_*: 9.97e-7 on the CPU emulator (libm expf / logf), 1.20e-6 on MI355X (both libraries) -> 4x the larger.
KERNEL_BAR = 4.8e-6
KERNEL_SHAPES_EMU = [(1, 320, 320, 0), (5, 321, 352, 0), (33, 1000, 1003, 0)]   # (rows, V, ldl, floats the base pointer is shifted by)
# a vocabulary with added tokens, an odd tail, and row starts that are not 16-byte aligned
KERNEL_SHAPES_GPU = KERNEL_SHAPES_EMU + [(3, 32000, 32000, 0), (130, 32003, 32064, 1)]
KINDS = ["first", "last", "random", "equal", "plus1e4", "minus1e4", "dominant", "mostly_ninf", "ninf_target"]


def _row(kind, V, rng):
    """-> (fp32 row, target, expected value or None)"""
    v = (rng.randn(V) * 3).astype(np.float32)
    t = int(rng.randint(0, V))
    want = None
    if kind == "first":
        t = 0
    elif kind == "last":
        t = V - 1
    elif kind == "equal":
        v[:] = np.float32(0.37)
        want = -np.log(float(V))
    elif kind == "plus1e4":
        v += np.float32(1e4)
    elif kind == "minus1e4":
        v -= np.float32(1e4)
    elif kind == "dominant":
        v[t] = np.float32(60.0)
        want = 0.0
    elif kind == "mostly_ninf":
        dead = rng.permutation(V)[: (9 * V) // 10]
        v[dead] = -np.inf
        v[t] = np.float32(1.5)
    elif kind == "ninf_target":
        v[t] = -np.inf
    return v, t, want


def check_token_logprob(be, rows, V, ldl, shift, seed=0):
    """every kind of row through launches of `rows` rows each; the pad columns V..ldl, the floats in front of the first row and behind
    the last hold NaN (one element read too many makes the result NaN).  -> largest |deviation| from float64 over the finite cases"""
    rng = np.random.RandomState(seed + rows * 7 + V)
    worst = 0.0
    n_launch = max(1, -(-len(KINDS) // rows))
    for launch in range(n_launch):
        kinds = [KINDS[(launch * rows + r) % len(KINDS)] for r in range(rows)]
        buf = np.full(shift + rows * ldl + 3, np.nan, dtype=np.float32)
        tgt = np.zeros(rows, dtype=np.int32)
        ref = np.zeros(rows, dtype=np.float64)
        exact = [None] * rows
        for r, kind in enumerate(kinds):
            v, t, exact[r] = _row(kind, V, rng)
            buf[shift + r * ldl: shift + r * ldl + V] = v
            tgt[r] = t
            v64 = v.astype(np.float64)
            with np.errstate(invalid="ignore"):
                ref[r] = v64[t] - np.logaddexp.reduce(v64)
        d_buf, d_tgt, d_out = be.f32(buf), be.i32(tgt), be.f32(np.full(rows, np.nan, dtype=np.float32))
        kc._call(be, "vck_token_logprob", d_buf[shift:], ldl, d_tgt, d_out, rows, V)
        got = be.host_f32(d_out).astype(np.float64)
        for r, kind in enumerate(kinds):
            what = f"token_logprob rows {rows} V {V} ldl {ldl} shift {shift} row {r} ({kind})"
            if kind == "ninf_target":
                assert got[r] == -np.inf, f"{what}: {got[r]}, expected -inf"
                continue
            assert np.isfinite(got[r]), f"{what}: {got[r]}"
            dev = abs(got[r] - ref[r])
            print(f"{what}: {got[r]:.7f} vs float64 {ref[r]:.7f} (|d| {dev:.2e})")
            worst = max(worst, dev)
            assert dev < KERNEL_BAR, f"{what}: deviates from float64 log-softmax by {dev}"
            if exact[r] is not None:
                assert abs(got[r] - exact[r]) < KERNEL_BAR + 1e-12, f"{what}: {got[r]}, expected {exact[r]}"
    return worst


# ---- engine / model against the reference's recorded label splice and loss ---------------------------------------------------
_CLASSES = {"vcoder_ds": lm.VCoderDSLlavaLlamaForCausalLM, "vcoder": lm.VCoderLlavaLlamaForCausalLM, "llava": lm.LlavaLlamaForCausalLM}
_models = {}


def model_for(variant, lib=None, operands="bf16", fmt="bf16", seed=42):
    """one model per (variant, library, weight format), shared by the tests of a module (the precision mode is set per use)"""
    key = (variant, id(lib), operands, fmt)
    if key not in _models:
        cfg = e2e_cases.tiny_cfg(variant)
        kw = {"_lib_override": lib} if lib is not None else {}
        m = _CLASSES[variant](cfg, device="cuda", operands=operands, **kw)
        m.engine.load_synthetic(seed)
        if fmt != "bf16":
            m.engine.set_weight_format(fmt)
        m.finalize_weights()
        _models[key] = m
    return _models[key]


def case_inputs(name):
    """-> (variant, ids, labels, images, segs, depths) of a case of score_cases.npz (pixels as its fixture's)"""
    g = np.load(os.path.join(e2e_cases.GOLD, str(SCORE[name + "__fixture"]) + ".npz"))
    variant = str(g["variant"])
    cfg = e2e_cases.tiny_cfg(variant)
    ids = SCORE[name + "__ids"]
    imgs, segs, deps = synth.synth_batch(ids.shape[0], cfg.vit_image_size)
    if bool(g["zero_depth"]):
        deps = np.zeros_like(deps)
    t = torch.from_numpy
    return (variant, ids, SCORE[name + "__labels"], t(imgs), t(segs) if bool(g["use_seg"]) else None,
            t(deps) if bool(g["use_depth"]) else None)


def logprob_bar(mode, name):
    """a log-prob is a logit minus a logsumexp, and each moves by at most the logit deviation the existing bar allows"""
    if mode in ("strict", "split"):
        return 2 * e2e_cases.TOL_STRICT
    return 2 * e2e_cases.REL_TOL_VS_FP32_REF * float(SCORE[name + "__max_abs_logit"])


def ref_logprobs(name):
    """float64 log-softmax of the reference's logits at its shifted spliced labels: from the committed fixture's prefill_logits where
    the case runs the fixture's own ids, else as recorded with the case"""
    new = SCORE[name + "__new_labels"]
    fx = str(SCORE[name + "__fixture"])
    g = np.load(os.path.join(e2e_cases.GOLD, fx + ".npz"))
    if not np.array_equal(g["input_ids"], SCORE[name + "__ids"]):
        return SCORE[name + "__ref_logprobs"]
    lg = torch.from_numpy(g["prefill_logits"]).double()
    lp = torch.log_softmax(lg[:, :-1], -1).numpy()
    out = np.zeros(new.shape, dtype=np.float64)
    for b, j in zip(*np.nonzero(new[:, 1:] != IGNORE)):
        out[b, j + 1] = lp[b, j, new[b, j + 1]]
    assert np.abs(out - SCORE[name + "__ref_logprobs"]).max() < 1e-5   # the generator ran the forward the fixture recorded
    return out


def check_case(name, model, mode="bf16"):
    """score() and forward(labels=) of one recorded case: spliced labels, zeros, log-probs, loss"""
    variant, ids, labels, imgs, segs, deps = case_inputs(name)
    model.engine.set_precision(mode)
    t = torch.from_numpy
    sc = model.score(t(ids), t(labels), images=imgs, segs=segs, depths=deps)
    new = SCORE[name + "__new_labels"]
    assert np.array_equal(sc.labels.numpy(), new), f"{name}: spliced labels differ from the reference's"
    lp = sc.token_logprobs.numpy()
    assert lp.dtype == np.float32 and lp.shape == new.shape
    scored = new != IGNORE
    scored[:, 0] = False
    assert (lp[~scored] == 0).all(), f"{name}: a position without a label (or position 0) carries a score"
    ref = ref_logprobs(name)
    bar = logprob_bar(mode, name)
    dev = float(np.abs(lp - ref)[scored].max()) if scored.any() else 0.0
    print(f"{name} [{mode}]: {int(scored.sum())} scored of {scored.size}, max |logprob - reference| {dev:.3e} (bar {bar:.3e})")
    assert dev < bar, f"{name} [{mode}]: token log-probs deviate by {dev} (bar {bar})"
    want = float(SCORE[name + "__loss"])
    out = model(input_ids=t(ids), labels=t(labels), images=imgs, segs=segs, depths=deps)
    for loss in (sc.loss, out.loss):
        assert loss.dtype == torch.float32 and loss.dim() == 0
        if np.isnan(want):
            assert bool(torch.isnan(loss)), f"{name}: loss {float(loss)}, the reference's is nan"
        else:
            print(f"{name} [{mode}]: loss {float(loss):.7f}, reference {want:.7f}")
            assert abs(float(loss) - want) < bar, f"{name} [{mode}]: loss {float(loss)} vs the reference's {want}"
    assert float(sc.loss) == float(out.loss) or (np.isnan(want) and bool(torch.isnan(out.loss)))
    assert np.allclose(sc.sequence_logprob.numpy(), lp.sum(1))
    assert out.logits.shape[:2] == new.shape   # logits are still returned
    tup = model(input_ids=t(ids), labels=t(labels), images=imgs, segs=segs, depths=deps, return_dict=False)
    assert tup[0].dim() == 0 and tup[1].shape == out.logits.shape   # the loss comes first (vcoder_ds_llava_llama.py:108-110)
    model.engine.set_precision("bf16")
    return dev


def own_logprobs(logits, labels):
    """float64 log-softmax of the engine's own all-row logits at the shifted labels (0 where nothing is scored)"""
    lp = torch.log_softmax(torch.as_tensor(np.asarray(logits)).double()[:, :-1], -1).numpy()
    out = np.zeros(labels.shape, dtype=np.float64)
    for b, j in zip(*np.nonzero(labels[:, 1:] != IGNORE)):
        out[b, j + 1] = lp[b, j, labels[b, j + 1]]
    return out


def check_against_own_logits(model, name, bar=KERNEL_BAR):
    """score() of a recorded case against log-softmax of that engine's own all_logits=True logits of the same call"""
    variant, ids, labels, imgs, segs, deps = case_inputs(name)
    t = torch.from_numpy
    out = model(input_ids=t(ids), labels=t(labels), images=imgs, segs=segs, depths=deps)
    sc = model.score(t(ids), t(labels), images=imgs, segs=segs, depths=deps)
    ref = own_logprobs(out.logits.numpy(), sc.labels.numpy())
    dev = float(np.abs(sc.token_logprobs.numpy() - ref).max())
    print(f"{name}: score() vs the engine's own all-row logits: {dev:.3e} (bar {bar:.3e})")
    assert dev < bar, f"{name}: score() deviates from the engine's own logits by {dev}"
    assert abs(float(sc.loss) - float(out.loss)) == 0.0
    return dev


# 2e-3: the bound of "last-row GEMV path disagrees with the all-rows GEMM path" (e2e_cases.check_fixture)
OWN_LOGITS_BAR = 2e-3 + KERNEL_BAR


def check_text_only(model, B, T, n_labelled_per_row, seed):
    """a text-only prefill with `n_labelled_per_row` labelled positions per row (None: all): score() and forward(labels=).loss against
    the engine's own all-row logits.  -> number of scored rows"""
    V = model.config.vocab_size
    rng = np.random.RandomState(seed)
    ids = rng.randint(3, V, size=(B, T)).astype(np.int64)
    labels = np.full((B, T), IGNORE, dtype=np.int64)
    for b in range(B):
        pos = np.arange(1, T) if n_labelled_per_row is None else rng.choice(np.arange(1, T), size=n_labelled_per_row, replace=False)
        labels[b, pos] = ids[b, pos]
    t = torch.from_numpy
    sc = model.score(t(ids), t(labels))
    assert np.array_equal(sc.labels.numpy(), labels)   # no placeholder in the row: the labels pass through
    out = model(input_ids=t(ids), labels=t(labels))
    ref = own_logprobs(out.logits.numpy(), labels)
    dev = float(np.abs(sc.token_logprobs.numpy() - ref).max())
    n = int((labels != IGNORE).sum())
    print(f"text-only B {B} T {T}: {n} scored rows, max deviation from the engine's own logits {dev:.3e}")
    assert dev < OWN_LOGITS_BAR, f"text-only B {B} T {T} ({n} scored rows): {dev}"
    assert float(sc.loss) == float(out.loss)
    assert abs(float(out.loss) + ref[labels != IGNORE].mean()) < OWN_LOGITS_BAR
    return n


# ---- candidates behind one prompt: extend + crop -------------------------------------------------------------------------------
def check_candidates(model, name="ds_img_depth_seg", mode="bf16", ns=(5, 70), logit_bar=None):
    """prefill a fixture prompt, score() two candidate continuations with crop between them; each against one labelled prefill of
    cat(prompt, candidate); the second candidate again on a fresh prefill: unchanged by the first having run"""
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    model.engine.set_precision(mode)
    t = lambda a: None if a is None else torch.from_numpy(a)
    B, T, V = ids.shape[0], ids.shape[1], cfg.vocab_size
    bar = 2 * (logit_bar if logit_bar is not None else
               (e2e_cases.TOL_STRICT if mode != "bf16" else e2e_cases.REL_TOL_VS_FP32_REF * float(np.abs(g["prefill_logits"]).max())))
    rng = np.random.RandomState(11)
    cands = [rng.randint(3, V, size=(B, n)).astype(np.int64) for n in ns]
    pre = model(input_ids=t(ids), images=t(imgs), segs=t(segs), depths=t(deps), use_cache=True)
    pkv = pre.past_key_values
    S = pkv.length
    got = []
    for c in cands:
        sc = model.score(t(c), t(c), past_key_values=pkv)
        assert pkv.length == S + c.shape[1]
        got.append(sc.token_logprobs.numpy().copy())
        assert (got[-1][:, 0] == 0).all() and np.array_equal(sc.labels.numpy(), c)
        pkv.crop(S)
        assert pkv.length == S
    # after crop the token selected on the device is stale: the state error, then an explicit token continues
    try:
        model.engine.decode_step(None)
        raise AssertionError("decode_step(tokens=None) after crop was not refused")
    except RuntimeError as e:
        assert "rewind" in str(e)
    for c, lp in zip(cands, got):
        full_ids = np.concatenate([ids, c], 1)
        labels = np.concatenate([np.full_like(ids, IGNORE), c], 1)
        labels[:, T] = IGNORE   # the candidate's first token is not scored by an extend chunk
        one = model.score(t(full_ids), t(labels), images=t(imgs), segs=t(segs), depths=t(deps))
        ref = one.token_logprobs.numpy()[:, -c.shape[1]:]
        dev = float(np.abs(lp - ref).max())
        print(f"candidate n = {c.shape[1]} [{mode}]: extend vs one labelled prefill {dev:.3e} (bar {bar:.3e})")
        assert dev < bar, f"candidate n = {c.shape[1]} [{mode}]: {dev}"
    pre = model(input_ids=t(ids), images=t(imgs), segs=t(segs), depths=t(deps), use_cache=True)
    alone = model.score(t(cands[1]), t(cands[1]), past_key_values=pre.past_key_values).token_logprobs.numpy()
    assert np.array_equal(alone, got[1]), "the second candidate's scores depend on the first having run"
    model.engine.set_precision("bf16")
    return S


def check_crop_then_decode(model, name="ds_img_depth_seg"):
    """prefill, two steps, crop back to the prompt, an explicit-token step: the logits of the first step again, and the oracle's"""
    import cpu_ref

    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    t = lambda a: None if a is None else torch.from_numpy(a)
    B = ids.shape[0]
    pre = model(input_ids=t(ids), images=t(imgs), segs=t(segs), depths=t(deps), use_cache=True)
    pkv = pre.past_key_values
    S = pkv.length
    tok = torch.from_numpy(np.random.RandomState(2).randint(3, cfg.vocab_size, size=(B, 1)))
    first = model(input_ids=tok, past_key_values=pkv, images=t(imgs)).logits.numpy().copy()
    model(input_ids=tok + 1, past_key_values=pkv, images=t(imgs))
    pkv.crop(S)
    again = model(input_ids=tok, past_key_values=pkv, images=t(imgs)).logits.numpy()
    assert np.array_equal(first, again), "a step behind crop() differs from the same step before it"
    om = cpu_ref.OracleModel(cfg, synth.synth_state_dict(cfg, int(g["seed"])), emu_bf16=True)
    _, cache = om.forward(ids.tolist(), t(imgs), t(segs), t(deps), last_only=True)
    o = cpu_ref.llama_forward(om.embed_tokens(tok.reshape(-1).tolist()).reshape(B, 1, -1), om.sd, om.cfg, cache, om.emu, last_only=True)
    assert float(np.abs(again[:, -1] - o[:, -1].numpy()).max()) < e2e_cases.TOL_VS_FP32_REF
    pkv.crop(S)
    many = model(input_ids=torch.cat([tok, tok + 1], 1), past_key_values=pkv)   # several ids behind a crop work as well
    assert many.logits.shape[1] == 2 and pkv.length == S + 2


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def check_refusals(model, name="ds_img_depth_seg"):
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    t = lambda a: None if a is None else torch.from_numpy(a)
    B, T, V = ids.shape[0], ids.shape[1], cfg.vocab_size
    kw = dict(images=t(imgs), segs=t(segs), depths=t(deps))
    pre = model(input_ids=t(ids), use_cache=True, **kw)
    pkv = pre.past_key_values
    tok = torch.from_numpy(np.random.RandomState(4).randint(3, V, size=(B, 1)))
    before = model(input_ids=tok, past_key_values=pkv, images=t(imgs)).logits.numpy().copy()
    pkv.crop(pkv.length - 1)
    bad = np.full((B, T), IGNORE, dtype=np.int64)
    text = np.nonzero(ids[0] >= 0)[0]
    bad[0, text[-1]] = V   # label 320 at a text position of the tiny model
    for call in (lambda: model(input_ids=t(ids), labels=t(bad), **kw),
                 lambda: model(input_ids=torch.cat([tok, tok], 1), labels=torch.tensor([[IGNORE, V]] * B), past_key_values=pkv)):
        try:
            call()
            raise AssertionError("a label outside the vocabulary was accepted")
        except IndexError:
            pass
    # straight at the engine as well (forward's own check sits in front of the continuation's)
    try:
        model.engine.prefill(ids, imgs, segs, deps, labels=bad)
        raise AssertionError("vc_prefill accepted a label outside the vocabulary")
    except IndexError:
        pass
    after = model(input_ids=tok, past_key_values=pkv, images=t(imgs)).logits.numpy()
    assert np.array_equal(before, after), "a refused call changed the cache of the previous KVCacheHandle"
    for shape in ((B, T + 1), (B + 1, T)):
        try:
            model(input_ids=t(ids), labels=torch.full(shape, IGNORE, dtype=torch.long), **kw)
            raise AssertionError("labels of another shape were accepted")
        except ValueError:
            pass
    try:
        model.engine.prefill(ids, imgs, segs, deps, labels=np.full((B, T + 1), IGNORE))
        raise AssertionError("HipEngine.prefill accepted labels of another shape")
    except ValueError:
        pass
    # a request followed by a failing prefill does not arm the next call
    eng = model.engine
    lab = np.full((B, T), IGNORE, dtype=np.int64)
    lab[:, text[-1]] = 5
    broken = ids.copy()
    broken[0, text[0]] = V + 7   # an id outside the vocabulary: IndexError out of the splice plan
    try:
        eng.prefill(broken, imgs, segs, deps, labels=lab)
        raise AssertionError("an id outside the vocabulary was accepted")
    except IndexError:
        pass
    import ctypes as C

    lp = np.full((B * 512,), 7.0, dtype=np.float32)   # what an armed request would overwrite
    eng.prefill(ids, imgs, segs, deps)
    assert eng.last_token_logprobs is None and (lp == 7.0).all()
    # ... also at the ABI: a request, a failing vc_prefill, then a plain one leaves the announced buffer alone
    rc = eng.lib.vc_request_token_scores(eng._model, lab.ctypes.data_as(C.c_void_p), B, T, lp.ctypes.data_as(C.c_void_p), None,
                                         C.c_size_t(lp.size))
    assert rc == 0
    try:
        eng.prefill(broken, imgs, segs, deps)
        raise AssertionError("an id outside the vocabulary was accepted")
    except IndexError:
        pass
    eng.prefill(ids, imgs, segs, deps)
    assert (lp == 7.0).all(), "a token-score request survived the failing prefill behind it"
    # too small a capacity, and a shape that does not match the call: VC_ERR_INVALID
    for (b_, t_, cap) in ((B, T, 3), (B, T + 1, lp.size)):
        lab2 = np.full((b_, t_), IGNORE, dtype=np.int64)
        assert eng.lib.vc_request_token_scores(eng._model, lab2.ctypes.data_as(C.c_void_p), b_, t_, lp.ctypes.data_as(C.c_void_p),
                                               None, C.c_size_t(cap)) == 0
        try:
            eng.prefill(ids, imgs, segs, deps)
            raise AssertionError("vc_prefill accepted a token-score request that does not fit it")
        except ValueError:
            pass
    # vc_rewind outside [prompt, position]
    _, _, S = eng.prefill(ids, imgs, segs, deps)
    for P in (S - 1, S + 1):
        try:
            eng.rewind(P)
            raise AssertionError("vc_rewind outside the live range was accepted")
        except ValueError:
            pass
    assert _lib.VC_ERR_STATE == -3
