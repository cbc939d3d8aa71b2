"""generate(num_return_sequences=n) on one prefill: cases shared by tests/test_fanout_emu.py (CPU emulator) and tests/test_gpu_fanout.py.

  vck_attention_fanout   against vck_attention_decode_rows on caches in which every row holds prefix + own tail: outputs equal as
                         values (an exactly-zero output may differ in sign), appended K / V rows equal, no other cache byte changed
  generate(num_return_sequences=n)
                         against the call on the prompt repeated n times (repeat_interleave, rows b n + j) with the same seed:
                         array_equal ids / n_generated / log-probs, through HipEngine.generate and model.generate
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

import kernel_cases as kc
import logprob_cases as lc
from kernel_cases import c_p
from speculate_cases import stream_round

model_for = lc.model_for


# ---- attention_fanout ------------------------------------------------------------------------------------------------------------
def keys_per_wave_instruction(hd, kv8):
    return 64 // (hd // (16 if kv8 else 8))


def prefix_lengths(hd, kv8):
    bt = stream_round(hd, kv8)
    return {"one": 1, "round-1": bt - 1, "round": bt, "round+1": bt + 1, "round+3kpw+1": bt + 3 * keys_per_wave_instruction(hd, kv8) + 1}


def tail_lengths(hd, kv8, P, S):
    bt = stream_round(hd, kv8)
    return {"first": 0, "one": 1, "cross": bt - (P % bt), "last": S - 1 - P}


def check_attention_fanout(be, hd, kv8, n, groups, H=2, S=None, seed=0):
    """groups: (P name or int, tail name or int, prefix row or None) per group — None: a free cache row of its own.  The cache has the
    G n rows of the launch plus one spare row per group; a group's prefix sits in its prefix row, which may be any row of the cache
    (its own first row, another of its rows, a row of the other group, a spare row): positions [0, P) of that row hold the prefix,
    positions >= P of every launch row that row's own tail — the two regions never overlap."""
    D = H * hd
    bt = stream_round(hd, kv8)
    S = S or 2 * bt + 100
    G = len(groups)
    R = G * n
    rows = R + G
    rng = np.random.RandomState(seed)
    Ps, poss, prow = [], [], []
    for g, (P, t, pr) in enumerate(groups):
        P = prefix_lengths(hd, kv8)[P] if isinstance(P, str) else P
        t = tail_lengths(hd, kv8, P, S)[t] if isinstance(t, str) else t
        Ps.append(P)
        poss.append(P + t)
        prow.append(R + g if pr is None else pr)
    assert all(1 <= Ps[g] <= poss[g] < S for g in range(G)), (Ps, poss, S)
    scale = 1.0 / math.sqrt(hd)
    cos, sin = kc.rope_tables(S, hd)
    qkv = kc._op_decode(kc._op_bits(kc.bf16_round(rng.randn(R, 3 * D)), be.operands), be.operands)
    prefix = rng.randn(G, H, S, hd).astype(np.float32)
    fan = rng.randn(rows, H, S, hd).astype(np.float32), rng.randn(rows, H, S, hd).astype(np.float32)   # K, V of the launch
    vprefix = rng.randn(G, H, S, hd).astype(np.float32)
    # descending P: a prefix row shared with another group's launch row keeps the longer prefix intact only behind the shorter tail
    # start — the cases place prefixes so that [0, P_g) of row prow[g] is read by group g alone or lies below every tail that row holds
    for g in range(G):
        fan[0][prow[g], :, :Ps[g]] = prefix[g, :, :Ps[g]]
        fan[1][prow[g], :, :Ps[g]] = vprefix[g, :, :Ps[g]]
    for g in range(G):   # a launch row used as a prefix row holds its own tail from ITS group's P on: the regions must not overlap
        if prow[g] < R:
            assert Ps[prow[g] // n] >= Ps[g], "the prefix would overlap the tail of the row that holds it"
    full = np.zeros((2, R, H, S, hd), np.float32)   # the reference's caches: row r = prefix of its group + its own tail
    for r in range(R):
        g = r // n
        for i, pre in enumerate((prefix, vprefix)):
            full[i, r] = fan[i][r]
            full[i, r, :, :Ps[g]] = pre[g, :, :Ps[g]]
    enc = (lambda a: kc._u8_dev(be, kc.e4m3_bytes(a))) if kv8 else (lambda a: be.bf16(a))
    cd, sd = be.f32(cos), be.f32(sin)
    fill = 0x3F80
    # ---- the fan-out launch
    kd, vd = enc(fan[0]), enc(fan[1])
    k_init, v_init = kc.raw_bits(kd).copy().reshape(rows, H, S, hd), kc.raw_bits(vd).copy().reshape(rows, H, S, hd)
    out = be.bits16(np.full((R, D), fill, np.uint16))
    rec = np.zeros((R, 4), np.int32)
    rec[:, 1] = np.repeat(poss, n)
    rd, pd, prd, qd = be.i32(rec), be.i32(Ps), be.i32(prow), be.bf16(qkv)
    rc = be.lib.vck_attention_fanout(be.ptr(qd), be.ptr(kd), be.ptr(vd), be.ptr(out), G, H, hd, S, n, rows, c_p(kc._addr(rd) + 4), 4,
                                     be.ptr(pd), be.ptr(prd), be.ptr(cd), be.ptr(sd), ctypes.c_float(scale), 3 if kv8 else 0, None)
    assert rc == 0
    be.sync()
    got = kc.raw_bits(out).reshape(R, D)
    gk, gv = kc.raw_bits(kd).reshape(rows, H, S, hd), kc.raw_bits(vd).reshape(rows, H, S, hd)
    # ---- the reference: the plain decode attention over R full rows
    kr, vr = enc(full[0]), enc(full[1])
    ro = be.bits16(np.full((R, D), fill, np.uint16))
    act = np.zeros((R, 4), np.int32)
    act[:, 0] = 1
    act[:, 1] = rec[:, 1]
    ad = be.i32(act)
    be.lib.vck_attention_decode_masked(be.ptr(qd), be.ptr(kr), be.ptr(vr), be.ptr(ro), R, H, hd, S, c_p(kc._addr(ad) + 4), 4, c_p(kc._addr(ad)),
                                       be.ptr(cd), be.ptr(sd), ctypes.c_float(scale), 3 if kv8 else 0, 0, None, 0, None)
    be.sync()
    ref = kc.raw_bits(ro).reshape(R, D)
    rk, rv = kc.raw_bits(kr).reshape(R, H, S, hd), kc.raw_bits(vr).reshape(R, H, S, hd)
    what = f"attention_fanout hd{hd} kv8={kv8} n{n} H{H} S{S} P {Ps} pos {poss} prefix rows {prow} [{be.operands}]"
    # outputs equal as values: array_equal on the floats (+0 == -0)
    gf, rf = kc._op_decode(got, be.operands), kc._op_decode(ref, be.operands)
    assert not np.isnan(rf).any() and (ref != fill).any(), f"{what}: the reference wrote nothing"
    assert np.array_equal(gf, rf), f"{what}: {np.count_nonzero(gf != rf)} output elements differ, first at {np.argwhere(gf != rf)[0]}"
    for r in range(R):
        p_ = poss[r // n]
        assert np.array_equal(gk[r, :, p_], rk[r, :, p_]) and np.array_equal(gv[r, :, p_], rv[r, :, p_]), f"{what}: appended row of {r} differs"
        k_init[r, :, p_] = gk[r, :, p_]
        v_init[r, :, p_] = gv[r, :, p_]
    assert np.array_equal(gk, k_init) and np.array_equal(gv, v_init), f"{what}: a cache byte outside the appended rows changed"


def fanout_kernel_cases():
    """(hd, kv8, n, groups): every P x tail length once per (hd, format) with n cycling through {2, 3, 4, 5, 8}, as two groups with
    different P and different prefix rows — group 0's prefix in a row of its own that is not its first (row 1), group 1's in a spare
    row — plus, per (hd, format), prefixes in the engine's placement (group g's in cache row g)."""
    cases = []
    ns = (2, 3, 4, 5, 8)
    i = 0
    for hd in (128, 64):
        for kv8 in (0, 1):
            names = list(prefix_lengths(hd, kv8))
            for a, P in enumerate(names):
                for t in ("first", "one", "cross", "last"):
                    n = ns[i % len(ns)]
                    i += 1
                    # group 0: prefix P in its own row 1; group 1: the next shorter prefix (or the same) in a spare row
                    Pa, Pb = prefix_lengths(hd, kv8)[P], prefix_lengths(hd, kv8)[names[a - 1]]
                    cases.append((hd, kv8, n, ((Pa, t, 1), (Pb, "one" if t != "one" else "first", None))))
            cases.append((hd, kv8, 4, (("round+1", "one", 0), ("round+1", "cross", 1))))    # the engine's rows: group g's prefix in row g
            cases.append((hd, kv8, 8, (("round+3kpw+1", "first", 0), ("round", "one", 1))))
    return cases


FANOUT_KERNEL_CASES = fanout_kernel_cases()
FANOUT_7B_CASES = [(128, kv8, 8, ((1216, 64, 0),), 4, 1344) for kv8 in (0, 1)]   # hd, kv8, n, groups, H, S


def check_attention_fanout_refused(be):
    """n outside 1 .. 8, a head dim without an instance, score rows beyond a CU's LDS: -1, nothing launched"""
    f = lambda hd, S, n, kv8: be.lib.vck_attention_fanout(None, None, None, None, 1, 1, hd, S, n, 1, None, 0, None, None, None, None,
                                                          ctypes.c_float(1.0), kv8, None)
    assert f(64, 4096, 9, 0) == -1 and f(64, 8192, 8, 1) == -1 and f(96, 256, 2, 0) == -1 and f(128, 256, 0, 0) == -1


# ---- generate(num_return_sequences=n) against the replicated call ----------------------------------------------------------------
MAX_NEW = 9
SEED = 11


def gen_inputs(B, V):
    """B prompts with different text and different images (the multimodal fixture prompts of the log-prob cases)"""
    ids, px = lc.inputs_for(max(B, 2), V)
    ids = ids[:B].copy()
    px = tuple(None if px.get(k) is None else px[k][:B] for k in ("images", "segs", "depths"))
    return ids, px


def rep(a, n):
    return None if a is None else np.repeat(np.asarray(a), n, axis=0)


def last_fanout(eng):
    return eng.last_fanout


_REF = {}


def replicated(eng, ids, px, n, K=0, **kw):
    """the definition of the result: the call on the prompts repeated n times -> (ids, log-probs)"""
    key = (id(eng), eng.precision, ids.tobytes(), n, K, repr(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _REF:
        new = eng.generate(rep(ids, n), *(rep(a, n) for a in px), logprobs=K > 0, top_logprobs=K, **kw)
        assert eng.last_fanout is None
        _REF[key] = (new, eng.last_generate_logprobs)
    new, lp = _REF[key]
    return new.copy(), None if lp is None else tuple(a.copy() for a in lp)


def check_equal(eng, B, n, K=3, shared=True, what="", **kw):
    """HipEngine.generate(num_return_sequences=n) equals the replicated call: ids (their column count is n_generated) and log-probs"""
    V = eng.cfg.vocab_size
    ids, px = gen_inputs(B, V)
    kw = dict(dict(max_new_tokens=MAX_NEW, do_sample=True, temperature=1.0, seed=SEED, fan_out=True), **kw)
    call_kw = {k: v for k, v in kw.items() if k != "fan_out"}
    ref, ref_lp = replicated(eng, ids, px, n, K=K, **call_kw)
    new = eng.generate(ids, *px, num_return_sequences=n, logprobs=K > 0, top_logprobs=K, **kw)
    w = f"generate(num_return_sequences={n}) B {B} {what} {sorted(kw)}"
    assert new.shape == ref.shape == (B * n, ref.shape[1]) and np.array_equal(new, ref), f"{w}: ids differ\n{new}\n{ref}"
    if K > 0:
        for got, want, name in zip(eng.last_generate_logprobs, ref_lp, ("token_logprobs", "top_logprobs", "top_ids")):
            assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), f"{w}: {name} differ"
    lf = eng.last_fanout
    assert lf == {"n": n, "shared": shared, "prefill_rows": B if shared else B * n}, f"{w}: last_fanout {lf}"
    return new, ref


def check_rows_differ(eng, n=5):
    new, _ = check_equal(eng, 1, n)
    assert len({tuple(r) for r in new.tolist()}) >= 2, f"temperature 1.0: the {n} rows are all the same\n{new}"


def check_eos_and_stop(eng, B=1, n=5):
    """the EOS id / a 2-id stop sequence is taken from the replicated call so that one row of a group finishes early while its group
    goes on"""
    V = eng.cfg.vocab_size
    ids, px = gen_inputs(B, V)
    base, _ = replicated(eng, ids, px, n, K=0, max_new_tokens=MAX_NEW, do_sample=True, temperature=1.0, seed=SEED)
    col = 3
    counts = {int(t): int((base[:, :MAX_NEW - 2] == t).any(1).sum()) for t in base[:, col]}
    eos = min(counts, key=lambda t: (counts[t], t))       # the id of column `col` that the fewest rows ever emit early
    assert 1 <= counts[eos] < B * n, f"no id finishes one row and leaves another running: {counts}"
    new, ref = check_equal(eng, B, n, eos_token_id=eos, pad_token_id=0, what="eos")
    done = [(r == eos).any() for r in ref[:, :-1]]
    assert any(done) and not all(done) and ref.shape[1] > col + 1, f"the replicated call does not show an early finish\n{ref}"
    for r, d in zip(ref, done):
        if d:
            assert (r[list(r).index(eos) + 1:] == 0).all(), "a finished row does not pad"
    r0 = next(r for r in base if r[col] == eos)
    check_equal(eng, B, n, stop_sequences=[[int(r0[col - 1]), int(r0[col])]], pad_token_id=0, what="stop sequence")


def check_processors(eng, B=2, n=4):
    from vcoder_amd import logits_processors as lp_

    check_equal(eng, B, n, processors=lp_.LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=2), what="processors")


def check_engine_fallbacks(eng, B=2, n=4):
    """fan_out=False and precision split: the same tensor, shared False"""
    check_equal(eng, B, n, shared=False, fan_out=False, what="fan_out=False")
    ids, px = gen_inputs(B, eng.cfg.vocab_size)
    eng.generate(ids, *px, max_new_tokens=2, do_sample=True, num_return_sequences=n)
    assert eng.last_fanout == {"n": n, "shared": False, "prefill_rows": B * n}, "fan_out defaults to False (profiles/fanout_wall_times.md)"
    eng.set_precision("split")
    try:
        check_equal(eng, 1, 2, shared=False, what="split")
    finally:
        eng.set_precision("bf16")
    new, ref = check_equal(eng, 1, 2, what="bf16 again")


def check_model_api(model, B=2, n=4):
    """model.generate(num_return_sequences=n): sequences [B n, T + L] rows b n + j carrying their prompt's input_ids, GenerateOutput
    fields B n rows wide, the streamer's columns B n wide — all equal to the replicated call's"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    t = torch.from_numpy(ids)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=-1, do_sample=True, temperature=1.0, seed=SEED, output_logprobs=True, top_logprobs=3)
    pk = lambda m: dict(images=None if px[0] is None else m(px[0]), segs=None if px[1] is None else m(px[1]), depths=None if px[2] is None else m(px[2]))
    rpt = lambda a: (a.repeat_interleave(n, 0) if torch.is_tensor(a) else np.repeat(a, n, axis=0))
    want = model.generate(t.repeat_interleave(n, 0), **kw, **pk(rpt))
    assert eng.last_fanout is None

    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got.append(v.clone())

        def end(self):
            pass

    s = Streamer()
    got = model.generate(t, num_return_sequences=n, fan_out=True, streamer=s, **kw, **pk(lambda a: a))
    assert eng.last_fanout == {"n": n, "shared": True, "prefill_rows": B}
    T = ids.shape[1]
    assert got.sequences.shape == (B * n, T + MAX_NEW) and torch.equal(got.sequences, want.sequences)
    assert torch.equal(got.sequences[:, :T], t.repeat_interleave(n, 0))
    for name in ("token_logprobs", "top_logprobs", "top_token_ids", "sequence_logprob"):
        assert got[name].shape[0] == B * n and torch.equal(got[name], want[name]), name
    assert all(v.shape[0] == B * n for v in s.got) and torch.equal(torch.stack(s.got[1:], 1), got.sequences[:, T:])
    bare = model.generate(t, num_return_sequences=n, fan_out=True, **{k: v for k, v in kw.items() if k not in ("output_logprobs", "top_logprobs")}, **pk(lambda a: a))
    assert isinstance(bare, torch.Tensor) and torch.equal(bare, want.sequences)
    return want, pk, t, kw


def check_model_fallbacks(model, B=2, n=4):
    """fan_out=False and a host-loop stopping criterion return the served call's tensor; last_fanout says not shared"""
    eng = model.engine
    want, pk, t, kw = check_model_api(model, B, n)
    off = model.generate(t, num_return_sequences=n, fan_out=False, **kw, **pk(lambda a: a))
    assert torch.equal(off.sequences, want.sequences) and eng.last_fanout["shared"] is False

    class HostCrit:   # no token-id form: the host loop
        def __call__(self, ids_, scores):
            return False

    kw2 = {k: v for k, v in kw.items() if k not in ("output_logprobs", "top_logprobs")}
    rpt = lambda a: (a.repeat_interleave(n, 0) if torch.is_tensor(a) else np.repeat(a, n, axis=0))
    host_want = model.generate(t.repeat_interleave(n, 0), stopping_criteria=[HostCrit()], **kw2, **pk(rpt))
    host = model.generate(t, num_return_sequences=n, fan_out=True, stopping_criteria=[HostCrit()], **kw2, **pk(lambda a: a))
    assert host.shape[0] == B * n and torch.equal(host, host_want)
    lf = eng.last_fanout
    assert lf is None or lf["shared"] is False


def check_arguments(model):
    import pytest

    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(1, V)
    t = torch.from_numpy(ids)
    kw = dict(max_new_tokens=4, eos_token_id=-1, images=px[0], segs=px[1], depths=px[2])
    with pytest.raises(ValueError, match="has to be 1, but is 3 when doing greedy search"):
        model.generate(t, num_return_sequences=3, **kw)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        model.generate(t, num_return_sequences=2, num_beams=2, **kw)
    with pytest.raises(ValueError):
        model.generate(t, num_return_sequences=17, do_sample=True, **kw)
    with pytest.raises(ValueError):
        eng.generate(ids, *px, max_new_tokens=4, do_sample=True, num_return_sequences=17)
    with pytest.raises(ValueError):
        eng.generate(ids, *px, max_new_tokens=4, do_sample=True, num_return_sequences=0)
    plain = model.generate(t, do_sample=True, seed=SEED, **kw)
    c0 = eng.step_captures()
    one = model.generate(t, do_sample=True, seed=SEED, num_return_sequences=1, **kw)
    assert isinstance(one, torch.Tensor) and torch.equal(one, plain) and eng.last_fanout is None
    assert eng.step_captures() == c0, "num_return_sequences=1 captured a step of its own"


def check_captures(eng, B=2):
    """two fan-out calls with the same (B, n) replay one capture; another n re-captures once; a plain call behind them is served by
    its own record"""
    V = eng.cfg.vocab_size
    ids, px = gen_inputs(B, V)
    kw = dict(max_new_tokens=MAX_NEW, do_sample=True, temperature=1.0, logprobs=True)
    plain = eng.generate(ids, *px, seed=SEED, **kw)            # the session loop's own step (a log-prob call): captured here
    eng.generate(ids, *px, seed=SEED, num_return_sequences=4, fan_out=True, **kw)
    c0 = eng.step_captures()
    a = eng.generate(ids, *px, seed=SEED + 1, num_return_sequences=4, fan_out=True, **kw)
    assert eng.step_captures() == c0, "a second fan-out call with the same (B, n) captured again"
    assert np.array_equal(eng.generate(ids, *px, seed=SEED, **kw), plain) and eng.step_captures() == c0, "a plain call between fan-out ones captured again"
    eng.generate(ids, *px, seed=SEED, num_return_sequences=2, fan_out=True, **kw)
    assert eng.step_captures() == c0 + 1, "another n must capture exactly one new step"
    assert a.shape[0] == B * 4


def check_session_closing(model, B=2, n=4):
    import pytest

    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    fresh = eng.generate(ids, *px, max_new_tokens=MAX_NEW, logprobs=True)
    new = eng.generate(ids, *px, max_new_tokens=5, do_sample=True, seed=SEED, num_return_sequences=n, fan_out=True)
    assert eng.last_fanout["shared"]
    with pytest.raises(RuntimeError, match="fan-out"):
        eng.decode_step(new[:, -1].astype(np.int32))
    with pytest.raises(RuntimeError, match="fan-out"):
        eng.extend(new[:, -2:].astype(np.int32))
    assert np.array_equal(eng.generate(ids, *px, max_new_tokens=MAX_NEW, logprobs=True), fresh)
    eng.prefill(ids, *px, has_attention_mask=True, reserve=4)   # the next prefill opens the loop again
    eng.clear_attention_mask()
    eng.decode_step(new[:B, 0].astype(np.int32))


def check_true_dims(batch_invariant, n=8, n_new=16, K=3):
    """7b dims, 2 decoder layers, the image prompt (S = 1216): B = 1, n = 8, 16 new tokens equal the replicated call.

    At these dims the prefill GEMMs of the replicated call (8 x 1216 rows) end in a split-K remainder round whose k-slices depend on
    the tile a row falls into: in the engine's default mode the replicated call gives its 8 identical prompts different prefill
    bits (measured on an MI355X: the step-0 top-logprob bits of its rows 6 and 7 differ from those of rows 0 .. 5; a shared prefix
    gave ids equal, 32 of 128 token log-probs different), so no shared prefix can equal it and the engine does not serve the
    request there: it repeats the prompts (shared False) and the equality holds as the replicated call's own.  Under
    set_batch_invariant(True) — no remainder round — the request is served and everything is array_equal."""
    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine

    cfg = vcfg.vicuna_7b("vcoder_ds")
    cfg.num_hidden_layers = 2
    cfg.vit_num_layers = 3
    eng = HipEngine(cfg)
    try:
        eng.load_synthetic(21)
        eng.finalize()
        eng.set_batch_invariant(bool(batch_invariant))
        ids = np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=0)])
        px = synth.synth_batch(1, 336)
        kw = dict(max_new_tokens=n_new, do_sample=True, temperature=1.0, seed=SEED, logprobs=True, top_logprobs=K)
        ref = eng.generate(rep(ids, n), *(rep(a, n) for a in px), **kw)
        ref_lp = eng.last_generate_logprobs
        assert int(eng.lib.vc_last_spliced_len(eng._model)) == 1216
        new = eng.generate(ids, *px, num_return_sequences=n, fan_out=True, **kw)
        for got, want, name in zip((new,) + eng.last_generate_logprobs, (ref,) + ref_lp, ("ids", "token_logprobs", "top_logprobs", "top_ids")):
            d = got.view(np.int32) != want.view(np.int32)
            print(f"7b dims n {n} batch_invariant={batch_invariant}: {name}: {int(d.sum())} of {d.size} entries differ")
        served = bool(batch_invariant)
        assert eng.last_fanout == {"n": n, "shared": served, "prefill_rows": 1 if served else n}, eng.last_fanout
        assert np.array_equal(new, ref), f"7b dims n {n}: ids differ\n{new}\n{ref}"
        for got, want, name in zip(eng.last_generate_logprobs, ref_lp, ("token_logprobs", "top_logprobs", "top_ids")):
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"7b dims n {n}: {name} differ"
    finally:
        eng.set_batch_invariant(False)   # (a switch of the root model)
        eng.close()
