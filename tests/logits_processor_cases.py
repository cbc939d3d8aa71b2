"""Logits processors inside the device decode loop (vck_logits_process, vc_request_logits_processors, generate(repetition_penalty=,
no_repeat_ngram_size=, min_new_tokens=, min_length=, bad_words_ids=)): the checks shared by the CPU-emulator tests
(tests/test_logits_processors_emu.py) and the `-m gpu` tests (tests/test_gpu_logits_processors.py).

The kernel's reference is `ref_process`, a numpy float32 restatement of HF 4.31's processors; the kernel must reproduce its bits.
tests/test_logits_processors_emu.py runs that restatement against Transformers' own classes where they import."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import e2e_cases
import kernel_cases as kc
import logprob_cases as lc
from score_cases import KERNEL_BAR
from vcoder_amd import _lib as vlib

# ---- kernel ------------------------------------------------------------------------------------------------------------------
KERNEL_SHAPES_EMU = [(1, 320, 320, 0), (5, 321, 352, 0), (2, 20, 24, 0)]   # (rows, V, ldl, shift)
KERNEL_SHAPES_GPU = KERNEL_SHAPES_EMU + [(3, 32000, 32000, 0), (9, 32003, 32064, 1)]
RS = dict(kc.RS, LP_PENALTY=15, LP_NGRAM=96, LP_MINNEW=97, LP_HIST_OFF=98, LP_HIST_LEN=99, LP_NBAD=100, LP_NEOS=101,
          LP_EOS=102)   # csrc/kernels.h RowStateField
MAX_BAD, MAX_BAD_LEN = 32, 8
SUBNORMAL = np.float32(1e-41)


def ref_process(raw, hist, penalty=1.0, ngram=0, bad_words=(), min_new=0, step=0, eos_ids=()):
    """numpy float32 restatement of the processors over one raw row [V] and its history (a list of ids): HF 4.31's order —
    RepetitionPenaltyLogitsProcessor (score < 0 ? score * p : score / p, read from the raw row), NoRepeatNGramLogitsProcessor,
    NoBadWordsLogitsProcessor, MinNewTokensLengthLogitsProcessor.  Ids outside [0, V) are skipped."""
    raw = np.asarray(raw, dtype=np.float32)
    V, L = raw.size, len(hist)
    out = raw.copy()
    p = np.float32(penalty)
    if p != np.float32(1.0):
        for t in {int(t) for t in hist if 0 <= t < V}:
            with np.errstate(all="ignore"):
                out[t] = raw[t] * p if raw[t] < 0 else raw[t] / p
    if ngram >= 1 and L + 1 >= ngram:
        tail = list(hist[L - ngram + 1:]) if ngram > 1 else []
        for i in range(L - ngram + 1):
            if list(hist[i:i + ngram - 1]) == tail and 0 <= hist[i + ngram - 1] < V:
                out[hist[i + ngram - 1]] = -np.inf
    for q in bad_words:
        pre = list(q[:-1])
        if (not pre or (len(pre) <= L and list(hist[L - len(pre):]) == pre)) and 0 <= q[-1] < V:
            out[q[-1]] = -np.inf
    if step < min_new:
        for e in eos_ids:
            if 0 <= e < V:
                out[e] = -np.inf
    return out


def _scenarios(V, rng):
    """-> list of dicts: prompt, gen (ids generated so far: step = len(gen)), penalty, ngram, bad (the row's own words), min_new, eos,
    eos_extra, raw (id -> value overrides), banned / kept (ids that must / must not end as -inf).  Tokens a .. f are distinct ids
    below V (V >= 20) and not 0 / V - 1, which the out-of-range scenario uses."""
    a, b, c, d, e, f, g = 3, 5, 7, 9, 11, 13, 15
    rnd = lambda n: [int(t) for t in rng.randint(0, V, size=n)]
    S = []

    def add(name, prompt, gen=(), penalty=1.0, ngram=0, bad=(), min_new=0, eos=-1, eos_extra=(), raw=None, banned=(), kept=()):
        S.append(dict(name=name, prompt=list(prompt), gen=list(gen), penalty=penalty, ngram=ngram, bad=[list(q) for q in bad],
                      min_new=min_new, eos=eos, eos_extra=list(eos_extra), raw=raw or {}, banned=list(banned), kept=list(kept)))

    add("all_off", rnd(5), rnd(3))
    add("prompt1_step0", [a], [], penalty=1.3, ngram=2, kept=[a])
    add("ngram_L=n-2", [a, a], [], ngram=4, kept=[a])
    add("ngram_L=n-1", [a, a], [a], ngram=4, kept=[a])                      # L + 1 >= n, but no start position yet
    add("ngram_L=n", [a, a], [a, a], ngram=4, banned=[a])                   # the first legal window: i = 0 = L - n
    add("ngram_periodic", [a, b, a, b], [a, b, a, b], penalty=0.7, ngram=3, banned=[a], kept=[b])   # overlapping matches
    h = rnd(1030)
    h[0], h[1], h[-1] = c, d, c
    add("ngram_long_i=0", h[:1000], h[1000:], penalty=1.3, ngram=2, banned=[d])                    # more than one pass, match at i = 0
    h = rnd(2500)
    h[-3:] = [e, e, e]
    add("ngram_long_i=L-n", h[:2000], h[2000:], ngram=3, banned=[e])                                # match at i = L - n
    add("ngram_n=1", [-200, 0, V - 1, V, a, a, b], [c, a], penalty=1.3, ngram=1, banned=[0, V - 1, a, b, c], kept=[d])
    vals = {a: np.float32(2.5), b: np.float32(-1.75), c: np.float32(0.0), d: np.float32(-0.0), e: np.float32(-np.inf), f: SUBNORMAL,
            g: -SUBNORMAL}
    for pen in (1.0, 1.3, 0.7):
        add(f"penalty_values_{pen}", [a, b, -200, c, V, d], [e, f, g, a, a], penalty=pen, raw=vals, kept=[a, b, c, d, f, g])
    add("penalised_and_banned", [a, b], [c], penalty=1.3, bad=[[a]], raw={a: np.float32(4.0)}, banned=[a], kept=[b, c])
    p10 = [a, b, c, d, e, f, g, a, c, e]
    add("bad_prefix_in_prompt", p10, [], bad=[[17], [p10[-1], 1], p10[-7:] + [2], [p10[-2], 4]], banned=[17, 1, 2], kept=[4])
    add("bad_prefix_straddles", [g, a, b, c, d], [e, f, g, a], bad=[[d, e, f, g, a, 1], [b, c, d, e, f, g, a, 2], [c, d, e, f, g, b, 4]],
        banned=[1, 2], kept=[4])                                             # 3 prompt ids + 4 generated ids in front of the last id
    add("bad_prefix_in_generated", [a, b, c], [d, e, f, g, a, b, c, d, e], bad=[[e, 1], [f, g, a, b, c, d, e, 2], [d, 4]],
        banned=[1, 2], kept=[4])
    add("bad_prefix_longer_than_history", [a, b, c], [], bad=[[a, a, a, a, a, b, c, 2], [c, 1]], banned=[1], kept=[2])
    add("bad_32_sequences", [a, b], [c, d], bad=[[16 + (i % 4)] if i < 16 else [d if i % 2 else a, i % 4] for i in range(32)],
        banned=[16, 17, 18, 19, 1, 3], kept=[0, 2])
    for neos, extra in ((1, []), (3, [b, V - 1])):
        add(f"min_new_step=m-1_{neos}eos", rnd(4), rnd(2), min_new=3, eos=a, eos_extra=extra, banned=[a] + extra)
        add(f"min_new_step=m_{neos}eos", rnd(4), rnd(3), min_new=3, eos=a, eos_extra=extra, raw={a: np.float32(1.0), b: np.float32(1.0)},
            kept=[a] + extra[:1])
    return S


def check_logits_process(be, rows, V, ldl, shift, seed=0):
    """every scenario through launches of `rows` rows each, rows of one launch with different settings; the bad-word table of a
    launch is the words of its rows one after the other (a row applies the table up to and including its own words).  The
    processed rows must hold the restatement's bits; pad columns, the floats in front of the first row and behind the last keep
    their NaN; the raw buffer is untouched."""
    rng = np.random.RandomState(seed + rows * 7 + V)
    scen = _scenarios(V, rng)
    seen_own = set()
    for launch in range(-(-len(scen) // rows)):
        use = [scen[(launch * rows + r) % len(scen)] for r in range(rows)]
        raw = np.full(shift + rows * ldl + 3, np.nan, dtype=np.float32)
        rec = kc.make_rows(rows)
        table, prompt, gen, words, own = [], [], [], [], []
        for r, s in enumerate(use):
            v = (rng.randn(V) * 3).astype(np.float32)
            for t, x in s["raw"].items():
                v[t] = x
            raw[shift + r * ldl: shift + r * ldl + V] = v
            if s["bad"] and len(table) + len(s["bad"]) <= MAX_BAD:
                table += s["bad"]
                nbad = len(table)
            else:   # (no words of its own, or no room for them: every other such row applies what the rows in front brought)
                nbad = len(table) if r % 2 else 0
            words.append([list(q) for q in table[:nbad]])
            own.append(words[-1] == s["bad"])
            rec[r, RS["STEP"]] = len(s["gen"])
            rec[r, RS["MAXNEW"]] = len(s["gen"]) + 2
            rec[r, RS["EOS"]] = s["eos"]
            rec[r, RS["OUT_OFF"]] = len(gen)
            rec[r, RS["LP_PENALTY"]] = kc._f32_bits(s["penalty"])
            rec[r, RS["LP_NGRAM"]] = s["ngram"]
            rec[r, RS["LP_MINNEW"]] = s["min_new"]
            rec[r, RS["LP_HIST_OFF"]] = len(prompt)
            rec[r, RS["LP_HIST_LEN"]] = len(s["prompt"])
            rec[r, RS["LP_NBAD"]] = nbad
            rec[r, RS["LP_NEOS"]] = len(s["eos_extra"])
            rec[r, RS["LP_EOS"]: RS["LP_EOS"] + len(s["eos_extra"])] = s["eos_extra"]
            prompt += s["prompt"]
            gen += s["gen"] + [V + 5, -7]   # what stands behind the ids generated so far is never read as history
        tab = np.zeros((MAX_BAD, 1 + MAX_BAD_LEN), dtype=np.int32)
        for q, w in enumerate(table):
            tab[q, 0] = len(w)
            tab[q, 1: 1 + len(w)] = w
        d_raw, d_out = be.f32(raw), be.f32(np.full_like(raw, np.nan))
        kc._call(be, "vck_logits_process", d_raw[shift:], ldl, d_out[shift:], ldl, be.i32(rec), be.i32(np.asarray(prompt + [0], np.int32)),
                 be.i32(np.asarray(gen, np.int32)), be.i32(tab), rows, V)
        got = be.host_f32(d_out)
        assert np.array_equal(be.host_f32(d_raw).view(np.int32), raw.view(np.int32)), "the raw rows were written"
        assert np.isnan(got[:shift]).all() and np.isnan(got[shift + rows * ldl:]).all(), "wrote in front of the first / behind the last row"
        for r, s in enumerate(use):
            what = f"logits_process rows {rows} V {V} ldl {ldl} shift {shift} launch {launch} row {r} ({s['name']})"
            row = got[shift + r * ldl: shift + (r + 1) * ldl]
            assert np.isnan(row[V:]).all(), f"{what}: pad columns written"
            v = raw[shift + r * ldl: shift + r * ldl + V]
            ref = ref_process(v, s["prompt"] + s["gen"], s["penalty"], s["ngram"], words[r], s["min_new"], len(s["gen"]),
                              [s["eos"]] + s["eos_extra"])
            bad = np.nonzero(row[:V].view(np.int32) != ref.view(np.int32))[0]
            assert bad.size == 0, f"{what}: ids {bad[:8]}: got {row[bad[:8]]}, restatement {ref[bad[:8]]}, raw {v[bad[:8]]}"
            if own[r]:   # the scenario shows what it is there to show
                seen_own.add(s["name"])
                assert all(ref[t] == -np.inf for t in s["banned"]), f"{what}: the restatement bans {np.nonzero(np.isneginf(ref))[0]}"
                assert all(ref[t] != -np.inf or v[t] == -np.inf for t in s["kept"]), f"{what}: the restatement bans a kept id"
            if s["name"] == "all_off" and not words[r]:
                assert np.array_equal(ref.view(np.int32), v.view(np.int32))
    assert rows > 1 or seen_own == {s["name"] for s in scen}, "a scenario never ran with exactly its own bad words"


# ---- the restatement against Transformers' own processors ------------------------------------------------------------------------
def check_restatement_against_hf(seed=0, V=97, trials=60):
    from transformers.generation import logits_process as hf

    rng = np.random.RandomState(seed)
    for trial in range(trials):
        L = int(rng.randint(1, 24))
        T = int(rng.randint(1, L + 1))
        hist = [int(t) for t in rng.randint(0, 6 if trial % 2 else V, size=L)]   # a small alphabet: repeats, n-gram matches
        raw = (rng.randn(V) * 3).astype(np.float32)
        raw[rng.randint(0, V, size=3)] = -np.inf
        raw[int(rng.randint(0, V))] = 0.0
        pen = float(rng.choice([1.3, 0.7, 2.0]))
        n = int(rng.randint(1, 5))
        eos = [int(t) for t in rng.choice(V, size=int(rng.randint(1, 4)), replace=False)]
        words = [[int(rng.randint(0, V))]] + [hist[L - k:] + [int(rng.randint(0, V))] for k in range(1, min(L, 7) + 1, 2)] + \
                [[int(t) for t in rng.randint(0, V, size=int(rng.randint(2, 9)))] for _ in range(3)]
        # (a word whose prefix is the WHOLE history: 4.31's _tokens_match bans its last id, as the kernel does; the
        # SequenceBiasLogitsProcessor of later releases ignores a word longer than the context.  Left out of the comparison.)
        words = [w for w in words if not (len(w) == 1 and w[0] in eos) and len(w) != L + 1]
        min_new, min_len = int(rng.randint(0, 6)), int(rng.randint(0, 30))
        ids, sc = torch.tensor([hist]), torch.from_numpy(raw)[None]
        step = L - T
        for what, proc, kw in (
                ("repetition penalty", hf.RepetitionPenaltyLogitsProcessor(pen), dict(penalty=pen)),
                ("no-repeat n-gram", hf.NoRepeatNGramLogitsProcessor(n), dict(ngram=n)),
                ("bad words", hf.NoBadWordsLogitsProcessor(words, eos_token_id=eos), dict(bad_words=words)),
                ("min new tokens", hf.MinNewTokensLengthLogitsProcessor(T, max(min_new, 1), eos_token_id=eos),
                 dict(min_new=max(min_new, 1), step=step, eos_ids=eos)),
                ("min length", hf.MinLengthLogitsProcessor(max(min_len, 1), eos_token_id=eos),
                 dict(min_new=max(min_len, 1) - T, step=step, eos_ids=eos))):
            want = proc(ids, sc.clone())[0].numpy()
            got = ref_process(raw, hist, **kw)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{what} trial {trial}: bans differ"
            assert np.array_equal(got, want), f"{what} trial {trial}: values differ"
        # the torch restatement the host loops use, all five at once, against HF's processors chained in 4.31's order
        from vcoder_amd import logits_processors as lp
        p = lp.make(pen, n, min_new, min_len, words, eos)
        want = sc.clone()
        chain = [hf.RepetitionPenaltyLogitsProcessor(pen), hf.NoRepeatNGramLogitsProcessor(n), hf.NoBadWordsLogitsProcessor(words, eos_token_id=eos)]
        if min_len > 0:
            chain.append(hf.MinLengthLogitsProcessor(min_len, eos_token_id=eos))
        if min_new > 0:
            chain.append(hf.MinNewTokensLengthLogitsProcessor(T, min_new, eos_token_id=eos))
        for proc in chain:
            want = proc(ids, want)
        # (HF penalises what the chain has not banned yet: both orders give the same row, -inf stays -inf under a positive factor)
        got = lp.apply_torch(p, ids, sc, T, eos)
        assert torch.equal(got, want), f"apply_torch trial {trial}"
        both = ref_process(raw, hist, pen, n, words, p.min_new_for(T), step, eos)
        assert np.array_equal(both, want[0].numpy()), f"all five, trial {trial}"


# ---- engine and model ------------------------------------------------------------------------------------------------------------
N_NEW = 6
model_for = lc.model_for


def inputs_for(B):
    """the multimodal prompt of the ds_img_depth_seg fixture (B = 2); B = 3: its rows 0, 1, 0 with one text id of the last row
    changed.  -> (ids [B, T] int64, kwargs of images / segs / depths)"""
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs("ds_img_depth_seg")
    if B == 3:
        pick = [0, 1, 0]
        ids = ids[pick].copy()
        text = np.nonzero(ids[2] >= 0)[0]
        ids[2, text[-1]] = (ids[2, text[-1]] + 17) % cfg.vocab_size
        imgs, segs, deps = (None if a is None else a[pick] for a in (imgs, segs, deps))
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    return ids, dict(images=t(imgs), segs=t(segs), depths=t(deps))


def _gen(model, ids, px, **kw):
    kw.setdefault("max_new_tokens", N_NEW)
    kw.setdefault("eos_token_id", -1)
    return model.generate(torch.from_numpy(ids), **px, **kw)


def configs_from(plain, T):
    """the processor settings of the end-to-end cases, derived from the ids `plain` [B, n] the call without processors generates so
    that every one of them has something to change: -> {name: (kwargs, baseline kwargs)}"""
    new = plain[:, T:].numpy()
    eos = int(new[0, 2])
    c = {
        "repetition_penalty": (dict(repetition_penalty=REP_PENALTY), {}),
        "no_repeat_ngram": (dict(no_repeat_ngram_size=NGRAM), {}),
        "bad_words": (dict(bad_words_ids=[[int(new[0, 0])], [int(new[1, 1]), int(new[1, 2])]]), {}),
        "min_new_tokens": (dict(min_new_tokens=5, eos_token_id=eos, pad_token_id=0), dict(eos_token_id=eos, pad_token_id=0)),
        "min_length": (dict(min_length=T + 5, eos_token_id=[eos, int(new[1, 1])], pad_token_id=0),
                       dict(eos_token_id=[eos, int(new[1, 1])], pad_token_id=0)),
    }
    c["all_five"] = (dict(repetition_penalty=REP_PENALTY, no_repeat_ngram_size=NGRAM, bad_words_ids=c["bad_words"][0]["bad_words_ids"],
                          min_new_tokens=5, min_length=T + 4, eos_token_id=eos, pad_token_id=0), dict(eos_token_id=eos, pad_token_id=0))
    return c


# chosen on the emulator (tiny vcoder_ds model, seed 42, the prompts of inputs_for) so that greedy decoding in every mode changes
# under each of them — which check_device_vs_host asserts
REP_PENALTY = 1.3
NGRAM = 2


def check_device_vs_host(model, mode, B):
    """1: greedy generate with each processor alone and all five together: the device loop returns what the host loop returns, and
    at least one row differs from the call without the processor"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T = ids.shape[1]
        plain = _gen(model, ids, px)
        bases = {"{}": plain}   # the calls without processors, each once
        for name, (kw, base_kw) in configs_from(plain, T).items():
            if repr(base_kw) not in bases:
                bases[repr(base_kw)] = _gen(model, ids, px, **base_kw)
            base = bases[repr(base_kw)]
            dev = _gen(model, ids, px, **kw)
            host = _gen(model, ids, px, processors_on_device=False, **kw)
            print(f"[{mode}] B {B} {name}: base {base[:, T:].tolist()} device {dev[:, T:].tolist()}")
            assert torch.equal(dev, host), f"[{mode}] B {B} {name}: device loop {dev[:, T:].tolist()}, host loop {host[:, T:].tolist()}"
            assert dev.shape != base.shape or not torch.equal(dev, base), f"[{mode}] B {B} {name}: the processor changes nothing: the case shows nothing"
    finally:
        eng.set_precision("bf16")


def finish_end(row, eos_ids):
    """columns of a generated row up to and including its finishing token"""
    for j, t in enumerate(row):
        if int(t) in eos_ids:
            return j + 1
    return len(row)


def assert_properties(what, prompt, new, ngram=0, bad_words=(), min_new=0, eos_ids=()):
    """2: what must hold of the ids whatever the model says — while the row is unfinished, no generated token completes an n-gram
    its history already holds, none completes a bad word, no EOS id comes before min_new tokens"""
    for b in range(new.shape[0]):
        row = [int(t) for t in new[b]]
        end = finish_end(row, set(eos_ids))
        seq = [int(t) for t in prompt[b]] + row[:end]
        T = len(prompt[b])
        for j in range(T, len(seq)):
            if ngram and j + 1 >= ngram:
                gram = seq[j + 1 - ngram: j + 1]
                assert all(seq[i: i + ngram] != gram for i in range(j + 1 - ngram)), f"{what} row {b}: the {ngram}-gram {gram} occurs twice in {seq}"
            for w in bad_words:
                assert seq[max(j + 1 - len(w), 0): j + 1] != list(w), f"{what} row {b}: bad word {w} in {seq}"
        assert not any(t in eos_ids for t in row[:min_new]), f"{what} row {b}: an EOS id among the first {min_new} tokens of {row}"


def check_properties(model, mode, B, sample):
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T = ids.shape[1]
        skw = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=11) if sample else {}
        plain = _gen(model, ids, px, **skw)[:, T:].numpy()
        w0 = int(plain[0, 0])
        other = lambda row: next(int(t) for t in row if int(t) != w0)   # (a bad word that is one EOS id is dropped, as HF drops it)
        eos = [other(plain[0, 1:]), other(plain[1, 2:])]
        words = [[w0], [int(plain[1, 0]), int(plain[1, 1])], [int(ids[0, -1]), w0]]
        for ngram in (1, 3):
            out = _gen(model, ids, px, no_repeat_ngram_size=ngram, bad_words_ids=words, min_new_tokens=4, eos_token_id=eos, pad_token_id=0,
                       **skw)
            new = out[:, T:].numpy()
            assert_properties(f"[{mode}] B {B} sample {sample} n {ngram}", ids, new, ngram, words, 4, eos)
            if sample:
                again = _gen(model, ids, px, no_repeat_ngram_size=ngram, bad_words_ids=words, min_new_tokens=4, eos_token_id=eos,
                             pad_token_id=0, **skw)
                assert torch.equal(out, again), "a sampled call does not repeat under its seed"
        # min_length counts the prompt ids: T + 3 asks for 3 new tokens, T - 1 for none
        out = _gen(model, ids, px, min_length=T + 3, eos_token_id=eos, pad_token_id=0, **skw)[:, T:].numpy()
        assert_properties(f"[{mode}] B {B} min_length", ids, out, min_new=3, eos_ids=eos)
        base = _gen(model, ids, px, eos_token_id=eos, pad_token_id=0, **skw)
        short = _gen(model, ids, px, min_length=T - 1, eos_token_id=eos, pad_token_id=0, **skw)
        assert torch.equal(short, base), "a min_length below the prompt length changes the ids"
    finally:
        eng.set_precision("bf16")


def check_with_logprobs(model, mode, B):
    """3: the ids are those of the processed call; the log-probs are those of the raw rows"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T = ids.shape[1]
        plain = _gen(model, ids, px)
        kw = configs_from(plain, T)["all_five"][0]
        kw = dict(kw, eos_token_id=-1, min_new_tokens=0, min_length=0)
        want = _gen(model, ids, px, **kw)
        assert not torch.equal(want, plain)
        out = _gen(model, ids, px, output_logprobs=True, top_logprobs=5, **kw)
        assert torch.equal(out.sequences, want), "the ids change with the log-prob request"
        new = out.sequences[:, T:].numpy()
        lg = lc.replay_logits(model, ids, px, new)
        tok_lp, top_lp, top_id = lc._np(out)
        worst = 0.0
        for s_ in range(new.shape[1]):
            for b in range(B):
                ids_ref, lp_ref, lse = lc.ref_topk(lg[s_, b], 5)
                dev = abs(float(tok_lp[b, s_]) - (float(lg[s_, b, new[b, s_]]) - lse))
                worst = max(worst, dev)
                assert dev < KERNEL_BAR, f"[{mode}] row {b} step {s_}: log-prob deviates from the raw row's log-softmax by {dev}"
                worst = max(worst, lc.compare_topk(f"[{mode}] row {b} step {s_}", lg[s_, b], 5, top_id[b, s_], top_lp[b, s_]))
        print(f"log-probs of a processed call [{mode}] B {B}: largest deviation from the raw rows {worst:.3e} (bar {KERNEL_BAR:.1e})")
        host = _gen(model, ids, px, output_logprobs=True, top_logprobs=5, processors_on_device=False, **kw)
        assert torch.equal(host.sequences, want) and torch.equal(host.top_token_ids, out.top_token_ids)
        assert np.abs(host.token_logprobs.numpy() - tok_lp).max() < 2 * KERNEL_BAR
    finally:
        eng.set_precision("bf16")


def check_no_leak(model, mode, B=2):
    """4: a plain generate behind a processed one returns what it returned before; a processed call that fails leaves no request"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T = ids.shape[1]
        plain = _gen(model, ids, px)
        kw = configs_from(plain, T)["all_five"][0]
        first = _gen(model, ids, px, **kw)
        assert not torch.equal(first, plain)
        assert torch.equal(_gen(model, ids, px), plain), "a plain generate behind a processed one differs"
        assert torch.equal(_gen(model, ids, px, **kw), first)
        try:
            _gen(model, ids, px, **dict(kw, max_new_tokens=model.config.max_position_embeddings))   # S + max_new over the capacity
            raise AssertionError("a call over the KV capacity was accepted")
        except (ValueError, RuntimeError, IndexError):
            pass
        assert torch.equal(_gen(model, ids, px), plain), "a processed call that failed left its request behind"
        # through the ABI: a request, then another entry point, then a plain generate
        a = (ids, px["images"], px["segs"], px["depths"])
        word, one = np.asarray([int(plain[0, T])], dtype=np.int32), np.asarray([1], dtype=np.int32)
        req = vlib.LogitsProcessors(1.0, 0, 0, 1, word.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 0, None)
        assert eng.lib.vc_request_logits_processors(eng._model, C.byref(req)) == 0
        eng.prefill(*a)
        assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a request outlived another entry point"
        assert eng.lib.vc_request_logits_processors(eng._model, C.byref(req)) == 0
        assert eng.lib.vc_request_logits_processors(eng._model, None) == 0
        assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a cancelled request fired"
        assert eng.lib.vc_request_logits_processors(eng._model, C.byref(req)) == 0
        assert not np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a request through the ABI alone does nothing"
    finally:
        eng.set_precision("bf16")


def check_refusals(model, B=2):
    """5: argument errors before the engine is touched, VC_ERR_INVALID from the C entry, VC_ERR_STATE from vc_generate_beam, beam
    search with a processor on the host loop"""
    eng = model.engine
    ids, px = inputs_for(B)
    T = ids.shape[1]
    plain = _gen(model, ids, px)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
               dict(no_repeat_ngram_size=-1), dict(bad_words_ids=[[]]), dict(bad_words_ids=[[3], []]), dict(bad_words_ids=[]),
               dict(min_new_tokens=-2), dict(min_length=-1), dict(num_beams=2, repetition_penalty=0.0)):
        try:
            _gen(model, ids, px, **kw)
            raise AssertionError(f"generate({kw}) was accepted")
        except ValueError:
            pass
    assert torch.equal(_gen(model, ids, px), plain)
    one = np.asarray([3, 4], dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lens = lambda *l: np.asarray(l, dtype=np.int32)
    many = np.zeros(40, dtype=np.int32)
    for req in (vlib.LogitsProcessors(0.0, 0, 0, 0, None, None, 0, None), vlib.LogitsProcessors(-1.3, 0, 0, 0, None, None, 0, None),
                vlib.LogitsProcessors(float("nan"), 0, 0, 0, None, None, 0, None), vlib.LogitsProcessors(float("inf"), 0, 0, 0, None, None, 0, None),
                vlib.LogitsProcessors(1.0, -1, 0, 0, None, None, 0, None),
                vlib.LogitsProcessors(1.0, 0, 0, 33, p(many), p(np.ones(33, dtype=np.int32)), 0, None),
                vlib.LogitsProcessors(1.0, 0, 0, 1, p(many), p(lens(9)), 0, None),
                vlib.LogitsProcessors(1.0, 0, 0, 2, p(one), p(lens(1, 0)), 0, None)):
        assert eng.lib.vc_request_logits_processors(eng._model, C.byref(req)) == -1
    a = (ids, px["images"], px["segs"], px["depths"])
    assert np.array_equal(eng.generate(*a, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a refused request changed the next call"
    # the device beam loop refuses a pending request (and consumes it)
    ok = vlib.LogitsProcessors(1.3, 0, 0, 0, None, None, 0, None)
    beam = eng.generate_beam(*a, num_beams=2, max_new_tokens=N_NEW)
    assert eng.lib.vc_request_logits_processors(eng._model, C.byref(ok)) == 0
    try:
        eng.generate_beam(*a, num_beams=2, max_new_tokens=N_NEW)
        raise AssertionError("vc_generate_beam ran with a vc_request_logits_processors pending")
    except RuntimeError as e:   # VC_ERR_STATE
        assert "logits processors" in str(e)
    again = eng.generate_beam(*a, num_beams=2, max_new_tokens=N_NEW)
    assert all(np.array_equal(x, y) for x, y in zip(beam, again))
    # model.generate(num_beams=2, <a processor>): the host loop
    plain_beam = _gen(model, ids, px, num_beams=2)
    words = [[int(plain_beam[0, T])]]
    out = _gen(model, ids, px, num_beams=2, repetition_penalty=REP_PENALTY, no_repeat_ngram_size=2, bad_words_ids=words)
    assert out.shape != plain_beam.shape or not torch.equal(out, plain_beam), "beam search ignores the processors"
    assert_properties("beam search", ids, out[:, T:].numpy(), 2, words)
    only = _gen(model, ids, px, num_beams=2, repetition_penalty=REP_PENALTY)
    assert only.shape != plain_beam.shape or not torch.equal(only, plain_beam), "beam search ignores repetition_penalty"
    assert torch.equal(_gen(model, ids, px, num_beams=2), plain_beam)


def check_streaming(model, B=2):
    """6: a streamer receives the processed ids"""
    ids, px = inputs_for(B)
    T = ids.shape[1]
    plain = _gen(model, ids, px)
    kw = dict(configs_from(plain, T)["all_five"][0], eos_token_id=-1, min_new_tokens=0, min_length=0)

    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got.append(v.clone())

        def end(self):
            pass

    for on_device in (True, False):
        s = Streamer()
        out = _gen(model, ids, px, streamer=s, processors_on_device=on_device, **kw)
        assert not torch.equal(out, plain)
        assert torch.equal(s.got[0], torch.from_numpy(ids))
        assert torch.equal(torch.stack(s.got[1:], 1), out[:, T:]), "the streamer saw other ids than the call returned"
