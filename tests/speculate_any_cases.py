"""Prompt-lookup speculation for sampled and processor-carrying calls (speculate_selection="any"): cases shared by
tests/test_speculate_any_emu.py (CPU emulator) and tests/test_gpu_speculate_any.py.

  vck_spec_select            against one 1-row vck_select_embed per verify row, the record's step raised by the row's index
  vck_logits_process_verify  against logits_processor_cases.ref_process over the history plus the drafts in front of the row
  vck_spec_accept_sel        against accept_ref_sel, speculate_cases.accept_ref with the selections given
  generate(speculate=k, speculate_selection="any") against the plain session loop of the same arguments and seed: array_equal ids /
                             log-probs, the counters against speculate_cases.simulate run on the plain call's own output
"""
from __future__ import annotations

import numpy as np
import torch

import kernel_cases as kc
import logits_processor_cases as pc
import speculate_cases as sc
from kernel_cases import RS, make_rows
from vcoder_amd import logits_processors as lp

model_for = sc.model_for
MAX_NEW = sc.MAX_NEW
SENTINEL = -7
SAMPLERS = {   # the CLI's setting, and one with every warper on
    "t0.2_k50": dict(do_sample=True, temperature=0.2, top_k=50),
    "t0.8_k20_p0.9": dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9),
}
SEED = 5


# ---- vck_spec_select -------------------------------------------------------------------------------------------------------------
def _select_records(B, steps, seed_lo):
    """records 0 .. 3: sampled T = 0.2 / top_k 50; greedy; sampled T = 1.0 / top_k 0 / top_p 0.9; top_p = 0 (the only_max branch)"""
    rows = make_rows(B, STEP=list(steps), MAXNEW=0, SEED_LO=seed_lo, SEED_HI=77)
    kinds = [dict(SAMPLE=1, INVTEMP=kc._f32_bits(1.0 / 0.2), TOPK=50), dict(SAMPLE=0),
             dict(SAMPLE=1, INVTEMP=kc._f32_bits(1.0), TOPK=0, TOPP=kc._f32_bits(0.9)), dict(SAMPLE=1, TOPK=0, TOPP=kc._f32_bits(0.0))]
    return rows, kinds


def check_spec_select(be, V, Q, lds=(-1,), seed=0):
    """B = 4 sequences with nq = (Q, Q, 2, 0) and different base steps; the four record kinds side by side in one launch, in two
    arrangements so that every kind owns Q rows once.  sel[b * Q + j] must be the next_tok of a 1-row vck_select_embed (advance 0, no
    embedding, EOS -1, no stops) on logits row b * Q + j with the record's STEP = step_b + j; rows j >= nq keep the sentinel; every
    lds_floats setting gives the same sel; another SEED_LO changes at least one sampled sel."""
    B, nq, steps = 4, [Q, Q, 2, 0], [3, 10, 0, 7]
    rng = np.random.RandomState(seed + V + Q)
    lg = (rng.randn(B * Q, V) * 2).astype(np.float32)
    lgd, nqd = be.f32(lg), be.i32(nq)
    sampled_sel = {}
    for rot in (0, 2):
        order = [(b + rot) % 4 for b in range(B)]   # the kind of record b
        for b in range(B):
            if order[b] == 1:   # greedy: an exact two-way tie at the maximum of every row, the lower id must win
                for j in range(Q):
                    r = lg[b * Q + j]
                    lo, hi = sorted(rng.choice(V, 2, replace=False))
                    r[lo] = r[hi] = np.float32(r.max() + 1.0)
        lgd = be.f32(lg)
        for seed_lo in (1234, 99):
            rows, kinds = _select_records(B, steps, seed_lo)
            for b in range(B):
                for k_, v_ in kinds[order[b]].items():
                    rows[b, RS[k_]] = v_
            rd = be.i32(rows)
            got = None
            for lf in lds:
                sel = be.i32(np.full(B * Q, SENTINEL))
                be.lib.vck_spec_select(be.ptr(lgd), V, V, be.ptr(rd), be.ptr(nqd), be.ptr(sel), B, Q, lf, None)
                be.sync()
                s_ = be.host_i32(sel).reshape(B, Q).copy()
                assert got is None or np.array_equal(s_, got), f"spec_select V {V} Q {Q}: lds_floats {lf} selects {s_}, {lds[0]} selected {got}"
                got = s_
            assert np.array_equal(be.host_i32(rd), rows), "spec_select wrote a record"
            if seed_lo == 1234:   # the reference: one plain selection per verify row
                out = be.zeros((4,), "i32")
                for b in range(B):
                    for j in range(Q):
                        if j >= nq[b]:
                            assert got[b, j] == SENTINEL, f"spec_select V {V} Q {Q}: row ({b}, {j}) behind its {nq[b]} queries was written"
                            continue
                        one = rows[b:b + 1].copy()
                        one[0, RS["STEP"]] = steps[b] + j
                        nxt, *_ = kc._select(be, lg[b * Q + j:b * Q + j + 1], one, out, 16, V, None, advance=0)
                        assert got[b, j] == nxt[0], f"spec_select V {V} Q {Q} rot {rot}: row ({b}, {j}) kind {order[b]}: {got[b, j]}, select_embed {nxt[0]}"
                        if order[b] == 1:
                            assert got[b, j] == int(np.argmax(lg[b * Q + j])), "the greedy record does not take the lower id of the tie"
                        if order[b] == 3:
                            assert got[b, j] == int(np.argmax(lg[b * Q + j])), "top_p = 0 keeps more than the maximum"
            sampled_sel[(rot, seed_lo)] = [got[b, j] for b in range(B) for j in range(nq[b]) if order[b] in (0, 2)]
    assert any(sampled_sel[(r, 1234)] != sampled_sel[(r, 99)] for r in (0, 2)), "another SEED_LO changes no sampled selection: an argmax would pass"
    return sampled_sel


# ---- the verify form of the logits processors -----------------------------------------------------------------------------------
def check_logits_process_verify(be, V, ldl, per_launch=5, seed=0):
    """the scenarios of logits_processor_cases with at least j + 1 generated ids, j in {1, 3, 7}: the last j generated ids leave the id
    store for the drafts of a token row; row i of the sequence must hold the bits of ref_process over prompt + the ids up to draft i with
    step = len(gen) - j + i (so row j is the plain launch over the whole history, row 0 the one j steps earlier).  Sequences with
    different settings share a launch; the raw buffer, the pad columns and the rows >= nq stay NaN / untouched."""
    rng = np.random.RandomState(seed + V)
    Q = 8
    seqs = [(s, j) for s in pc._scenarios(V, rng) for j in (1, 3, 7) if len(s["gen"]) >= j + 1]
    assert {j for _, j in seqs} == {1, 3, 7} and len(seqs) >= 12
    for at in range(0, len(seqs), per_launch):
        use = seqs[at:at + per_launch]
        B = len(use)
        raw = np.full(B * Q * ldl + 3, np.nan, dtype=np.float32)
        rec = make_rows(B)
        table, prompt, gen, words = [], [], [], []
        tok, nq = np.full((B, Q), 2, np.int32), np.zeros(B, np.int32)
        for b, (s, j) in enumerate(use):
            n = len(s["gen"]) - j   # ids in the store
            for i in range(j + 1):
                v = (rng.randn(V) * 3).astype(np.float32)
                for t, x in s["raw"].items():
                    v[t] = x
                raw[(b * Q + i) * ldl:(b * Q + i) * ldl + V] = v
            if s["bad"] and len(table) + len(s["bad"]) <= pc.MAX_BAD:
                table += s["bad"]
                nbad = len(table)
            else:
                nbad = len(table) if b % 2 else 0
            words.append([list(q) for q in table[:nbad]])
            rec[b, RS["STEP"]] = n
            rec[b, RS["MAXNEW"]] = len(s["gen"]) + 2
            rec[b, RS["EOS"]] = s["eos"]
            rec[b, RS["OUT_OFF"]] = len(gen)
            rec[b, pc.RS["LP_PENALTY"]] = kc._f32_bits(s["penalty"])
            rec[b, pc.RS["LP_NGRAM"]] = s["ngram"]
            rec[b, pc.RS["LP_MINNEW"]] = s["min_new"]
            rec[b, pc.RS["LP_HIST_OFF"]] = len(prompt)
            rec[b, pc.RS["LP_HIST_LEN"]] = len(s["prompt"])
            rec[b, pc.RS["LP_NBAD"]] = nbad
            rec[b, pc.RS["LP_NEOS"]] = len(s["eos_extra"])
            rec[b, pc.RS["LP_EOS"]: pc.RS["LP_EOS"] + len(s["eos_extra"])] = s["eos_extra"]
            prompt += s["prompt"]
            gen += s["gen"][:n] + [V + 5, -7]   # what stands behind the ids in the store is never read as history
            tok[b, 0], tok[b, 1:1 + j], nq[b] = s["gen"][n - 1], s["gen"][n:], j + 1
        tab = np.zeros((pc.MAX_BAD, 1 + pc.MAX_BAD_LEN), dtype=np.int32)
        for q, w in enumerate(table):
            tab[q, 0] = len(w)
            tab[q, 1: 1 + len(w)] = w
        d_raw, d_out = be.f32(raw), be.f32(np.full_like(raw, np.nan))
        args = [be.i32(a) for a in (rec, np.asarray(prompt + [0], np.int32), np.asarray(gen, np.int32), tab, tok, nq)]   # (held until the sync)
        be.lib.vck_logits_process_verify(be.ptr(d_raw), ldl, be.ptr(d_out), ldl, *(be.ptr(a) for a in args), B, Q, V, None)
        be.sync()
        got = be.host_f32(d_out)
        assert np.array_equal(be.host_f32(d_raw).view(np.int32), raw.view(np.int32)), "the raw rows were written"
        assert np.isnan(got[B * Q * ldl:]).all(), "wrote behind the last row"
        for b, (s, j) in enumerate(use):
            n = len(s["gen"]) - j
            for i in range(Q):
                what = f"logits_process_verify V {V} ldl {ldl} sequence {at + b} ({s['name']}, j {j}) row {i}"
                row = got[(b * Q + i) * ldl:(b * Q + i + 1) * ldl]
                if i > j:
                    assert np.isnan(row).all(), f"{what}: a row behind the sequence's queries was written"
                    continue
                assert np.isnan(row[V:]).all(), f"{what}: pad columns written"
                v = raw[(b * Q + i) * ldl:(b * Q + i) * ldl + V]
                ref = pc.ref_process(v, s["prompt"] + s["gen"][:n + i], s["penalty"], s["ngram"], words[b], s["min_new"], n + i,
                                     [s["eos"]] + s["eos_extra"])
                bad = np.nonzero(row[:V].view(np.int32) != ref.view(np.int32))[0]
                assert bad.size == 0, f"{what}: ids {bad[:8]}: got {row[bad[:8]]}, restatement {ref[bad[:8]]}, raw {v[bad[:8]]}"
                if i == j and words[b] == s["bad"]:   # the whole history: the scenario shows what it is there to show
                    assert all(ref[t] == -np.inf for t in s["banned"]) and all(ref[t] != -np.inf or v[t] == -np.inf for t in s["kept"]), what


# ---- vck_spec_accept_sel -----------------------------------------------------------------------------------------------------------
def accept_ref_sel(r, sel, tok, nq):
    """speculate_cases.accept_ref with the rows' selections given in place of the argmax"""
    if nq <= 0:
        return None, [0, 0, 0, 0]
    emitted, last = 0, int(tok[0])
    for j in range(nq):
        if j > 0 and int(tok[j]) != int(sel[j - 1]):
            break
        last = sc.emit_ref(r, int(sel[j]))
        r["step"] += 1
        r["pos"] += 1
        emitted += 1
        if r["finished"] or r["step"] >= r["max_new"]:
            break
    return last, [1, emitted, nq - 1, emitted - 1]


def check_spec_accept_sel(be, logprobs=False):
    """the cases of speculate_cases.ACCEPT_CASES with sel = their `argmax per row` list over logits whose argmax is something else (so a
    kernel that still reduces the rows fails), NaN in the rows of one sequence (nothing of the logits is read); lp_tok slots hold the
    chosen scratch, the top-K slots the scratch rows"""
    names = list(sc.ACCEPT_CASES)
    B, Q, V, pad, stride, K = len(names), 4, sc.V_SMALL, 3, 16, 3
    rng = np.random.RandomState(6)
    lg = rng.randn(B, Q, V).astype(np.float32)
    lg[:, :, 60] = 50.0    # every row's argmax: an id no case selects
    lg[0] = np.nan
    rows = make_rows(B, PAD=pad, OUT_OFF=[b * stride for b in range(B)], MAXNEW=12)
    out = np.full((B, stride), pad, np.int32)
    toks, nqs, sels, recs = np.zeros((B, Q), np.int32), np.zeros(B, np.int32), np.zeros((B, Q), np.int32), []
    for b, name in enumerate(names):
        tok, nq, want, f, _ = sc.ACCEPT_CASES[name]
        toks[b], nqs[b], sels[b] = tok, nq, want
        gen = list(f.get("gen", [1, tok[0]]))
        if "step" in f:
            gen = gen[:f["step"]]
        r = dict(step=len(gen), pos=100 + b, finished=0, eos=f.get("eos", -1), pad=pad, stops=f.get("stops", []),
                 tail=f.get("tail", [-(2 ** 31)] * 7), out=gen + [pad] * (stride - len(gen)), max_new=f.get("max_new", 12))
        recs.append(r)
        rows[b, RS["STEP"]], rows[b, RS["POS"]], rows[b, RS["EOS"]], rows[b, RS["MAXNEW"]] = r["step"], r["pos"], r["eos"], r["max_new"]
        rows[b, RS["NSTOP"]] = len(r["stops"])
        rows[b, RS["TAIL"]:RS["TAIL"] + 7] = r["tail"]
        for i, q in enumerate(r["stops"]):
            rows[b, RS["STOP"] + 9 * i] = len(q)
            rows[b, RS["STOP"] + 9 * i + 1: RS["STOP"] + 9 * i + 1 + len(q)] = q
        out[b, :len(gen)] = gen
    assert (sels != 60).all()
    rd, od, nxt, cnt = be.i32(rows), be.i32(out), be.i32(np.full(B, -7)), be.i32(np.tile([10, 20, 30, 40], (B, 1)))
    lgd, td, nd, sd = be.f32(lg.reshape(B * Q, V)), be.i32(toks), be.i32(nqs), be.i32(sels)
    s_lp = s_id = s_ch = lp_tok = lp_top = lp_ids = None
    if logprobs:
        s_lp_h, s_id_h = rng.randn(B * Q, K + 1).astype(np.float32), rng.randint(0, V, (B * Q, K + 1)).astype(np.int32)
        s_ch_h = rng.randn(B * Q).astype(np.float32) - 20.0   # no entry of the top-K scratch
        s_lp, s_id, s_ch = be.f32(s_lp_h), be.i32(s_id_h), be.f32(s_ch_h)
        lp_tok, lp_top, lp_ids = be.f32(np.full((B * stride,), 7.0)), be.f32(np.full((B * stride, K), 7.0)), be.i32(np.full((B * stride, K), -7))
    be.lib.vck_spec_accept_sel(be.ptr(lgd), V, V, be.ptr(rd), be.ptr(nxt), be.ptr(od), be.ptr(td), be.ptr(nd), B, Q, be.ptr(cnt), be.ptr(s_lp),
                               be.ptr(s_id), K + 1, be.ptr(lp_tok), be.ptr(lp_top), be.ptr(lp_ids), K if logprobs else 0, be.ptr(sd), be.ptr(s_ch), None)
    be.sync()
    g_rows, g_out, g_nxt, g_cnt = be.host_i32(rd), be.host_i32(od), be.host_i32(nxt), be.host_i32(cnt)
    emitted_of = {}
    for b, name in enumerate(names):
        r = recs[b]
        step0 = r["step"]
        last, c = accept_ref_sel(r, sels[b], toks[b], int(nqs[b]))
        emitted_of[name] = c[1]
        w = f"spec_accept_sel {name}"
        assert list(g_out[b]) == r["out"], f"{w}: ids {list(g_out[b])}, want {r['out']}"
        assert (g_rows[b, RS["STEP"]], g_rows[b, RS["POS"]], g_rows[b, RS["FINISHED"]]) == (r["step"], r["pos"], r["finished"]), \
            f"{w}: step / pos / finished {g_rows[b, 1:4]}, want {r['step']} {r['pos']} {r['finished']}"
        assert g_nxt[b] == last and list(g_cnt[b]) == [10 + c[0], 20 + c[1], 30 + c[2], 40 + c[3]], f"{w}: next {g_nxt[b]} counters {g_cnt[b]}"
        if logprobs:
            t, tp, ti = be.host_f32(lp_tok).reshape(B, stride), be.host_f32(lp_top).reshape(B, stride, K), be.host_i32(lp_ids).reshape(B, stride, K)
            for s_ in range(stride):
                j = s_ - step0
                if 0 <= j < c[1]:
                    assert t[b, s_] == s_ch_h[b * Q + j] and np.array_equal(tp[b, s_], s_lp_h[b * Q + j, :K]) and \
                        np.array_equal(ti[b, s_], s_id_h[b * Q + j, :K]), f"{w}: log-prob slot {s_}"
                else:
                    assert t[b, s_] == 7.0 and (tp[b, s_] == 7.0).all() and (ti[b, s_] == -7).all(), f"{w}: slot {s_} was written"
    # the selections decide, not the rows: the two tie cases accept their whole run
    want = dict(all_accepted=4, none_accepted=1, some_accepted=3, no_drafts=1, eos_inside_run=2, stop_completed_inside_run=2,
                stop_with_history=1, max_new_cut=2, argmax_tie_lower_id_wins=4, argmax_tie_higher_id_loses=4)
    assert emitted_of == want, f"the cases no longer show what they are named for: {emitted_of}"


# ---- generate(speculate=k, speculate_selection="any") against the plain session loop ------------------------------------------------
def _counters(sp):
    return np.stack([sp["steps"], sp["tokens"], sp["drafted"], sp["accepted"]], 1)


def check_generate(model, k, B, lookup="truth", ng=2, K=0, max_new=MAX_NEW, eos_from=None, stop_from=None, selection="any", **kw):
    """ids and log-probs array_equal to the plain session loop of the same arguments and seed; the counters equal
    speculate_cases.simulate run on the plain call's own output.  kw: the sampling arguments and / or `processors`.  The lookup ids
    derive from the plain output of the call without EOS / stop; eos_from / stop_from: the EOS id / a 2-id stop sequence is taken
    from that column of row 0 of that output.  -> (counters dict, plain ids, captures added)"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    kw = dict(kw, max_new_tokens=max_new)
    base, _ = sc.session_reference(eng, ids, px, **kw)
    if eos_from is not None:
        kw.update(eos_token_id=int(base[0, eos_from]), pad_token_id=0)
    if stop_from is not None:
        kw.update(stop_sequences=[[int(base[0, stop_from - 1]), int(base[0, stop_from])]], pad_token_id=0)
    ref, ref_lp = sc.session_reference(eng, ids, px, K=K, **kw)
    look = sc.lookups(lookup, base, V, seed=k + B)
    steps0 = eng.step_captures()
    new = eng.generate(ids, *px, speculate=k, speculate_selection=selection, lookup_ngram=ng, lookup_ids=look, logprobs=K > 0, top_logprobs=K, **kw)
    what = f"generate(speculate={k}, {selection!r}) B {B} lookup {lookup} {sorted(kw)} eos_from {eos_from} stop_from {stop_from}"
    assert new.shape == ref.shape and np.array_equal(new, ref), f"{what}: ids differ\n{new}\n{ref}"
    sp = eng.last_speculation
    assert sp is not None, f"{what}: the request was not served"
    if K > 0:
        for got, want, name in zip(eng.last_generate_logprobs, ref_lp, ("token_logprobs", "top_logprobs", "top_ids")):
            assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), f"{what}: {name} differ"
    if stop_from is None:
        full = np.where(np.arange(max_new)[None] < ref.shape[1], np.pad(ref, ((0, 0), (0, max_new - ref.shape[1]))), 0)
        want = sc.expected_counters(ids, full, look, k, ng, V, kw.get("eos_token_id", -1))
        assert np.array_equal(_counters(sp), want), f"{what}: counters {_counters(sp).tolist()}, simulated {want.tolist()}"
    return sp, ref, eng.step_captures() - steps0


def check_sampled(model, sampler, k, B, K=5, seed=SEED):
    """lookup_ids = the plain sampled output, that output with every third id replaced, none.  That the truth saves steps and that the
    corrupted lookup is accepted in part are properties of the inputs: they are established by simulating on the plain output alone,
    then the engine's counters must equal the simulation (check_generate)."""
    eng, V = model.engine, model.config.vocab_size
    kw = dict(SAMPLERS[sampler], seed=seed)
    ids, px = sc.gen_inputs(B, V)
    truth, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW, **kw)
    greedy, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW)
    sim = {kind: sc.expected_counters(ids, truth, sc.lookups(kind, truth, V, seed=k + B), k, 2, V) for kind in ("truth", "corrupted")}
    assert (sim["truth"][:, 0] < MAX_NEW - 1).all(), f"seed {seed}: the truth as lookup saves no step in the simulation: {sim['truth'].tolist()}"
    assert 0 < sim["corrupted"][:, 3].sum() < sim["corrupted"][:, 2].sum(), f"seed {seed}: corrupted lookup, simulated {sim['corrupted'].tolist()}"
    for kind in ("truth", "corrupted", "none"):
        sp, ref, _ = check_generate(model, k, B, lookup=kind, K=K, **kw)
        assert np.array_equal(ref, truth)
        if kind == "truth":
            assert (sp["steps"] < MAX_NEW - 1).all() and (sp["tokens"] == MAX_NEW - 1).all()
        if kind == "corrupted":
            assert 0 < sp["accepted"].sum() < sp["drafted"].sum()
    return not np.array_equal(truth, greedy)


def biting_ngram(ids, plain):
    """the largest no-repeat n-gram size in 3 .. 1 under which some generated token of `plain` (behind its first: the verify steps)
    completes an n-gram its history (prompt + generated ids) already holds — the size that changes this output"""
    for n in (3, 2, 1):
        for b in range(plain.shape[0]):
            seq = [int(t) for t in ids[b]] + [int(t) for t in plain[b]]
            T = ids.shape[1]
            for j in range(T + 1, len(seq)):
                gram = seq[j + 1 - n: j + 1]
                if any(seq[i: i + n] == gram for i in range(j + 1 - n)):
                    return n
    raise AssertionError("no generated id of the plain output repeats an id of its history")


def processor_sets(model, B, kw):
    """-> {name: (processors, extra call kwargs, baseline kwargs)}: each set derived from the plain output of the call with `kw` (and the
    baseline kwargs) so that it has something to change inside the verify steps"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    plain, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW, **kw)
    eos = int(plain[0, 3])
    word = [[int(plain[0, 4])]]
    ngram = biting_ngram(ids, plain)
    e = dict(eos_token_id=eos, pad_token_id=0)
    return {
        "repetition_penalty": (lp.make(1.3), {}, {}),
        "no_repeat_ngram": (lp.make(None, ngram), {}, {}),
        "bad_word": (lp.make(bad_words_ids=word), {}, {}),
        "min_new_tokens": (lp.make(min_new_tokens=7, eos_ids=[eos]), e, e),
        "all": (lp.make(1.3, ngram, 7, None, word, [eos]), e, e),
    }


def check_processors(model, name, sample, k=3, B=2):
    """a processor set, greedy or sampled: the plain processed output differs from the processor-free one (else the case shows
    nothing), and the speculated call — its own plain output as lookup — returns it"""
    eng, V = model.engine, model.config.vocab_size
    kw = dict(SAMPLERS["t0.2_k50"], seed=SEED) if sample else {}
    proc, extra, base_kw = processor_sets(model, B, kw)[name]
    ids, px = sc.gen_inputs(B, V)
    free, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW, **kw, **base_kw)
    own, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW, processors=proc, **kw, **extra)
    assert own.shape != free.shape or not np.array_equal(own, free), f"{name} sample {sample}: the processors change nothing: the case shows nothing"
    sp, ref, _ = check_generate(model, k, B, lookup="truth", K=5, processors=proc, **kw, **extra)
    assert np.array_equal(ref, own) and sp["accepted"].sum() > 0
    check_generate(model, k, B, lookup="corrupted", processors=proc, **kw, **extra)
    return sp


def check_eos_and_stop(model, k=3, B=2):
    """an EOS id and a two-id stop sequence completed inside an accepted run, under sampling"""
    kw = dict(SAMPLERS["t0.8_k20_p0.9"], seed=SEED)
    sp, ref, _ = check_generate(model, k, B, lookup="truth", K=3, eos_from=6, **kw)
    assert (ref[0, 7:] == 0).all() and sp["accepted"][0] > 0, "the EOS id does not end row 0 at column 6, or nothing was accepted in front of it"
    sp, ref, _ = check_generate(model, k, B, lookup="truth", stop_from=6, **kw)
    assert sp["accepted"].sum() > 0
    check_generate(model, k, B, lookup="none", eos_from=6, **kw)


def check_num_return_sequences(model, k=3, B=2, n=2):
    """the repeated-prompt form: array_equal to the call without speculation, counters for B n rows"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    kw = dict(SAMPLERS["t0.2_k50"], seed=SEED, max_new_tokens=MAX_NEW, num_return_sequences=n)
    ref = eng.generate(ids, *px, logprobs=True, top_logprobs=3, **kw)
    ref_lp = eng.last_generate_logprobs
    assert eng.last_speculation is None and ref.shape[0] == B * n
    look = [list(map(int, ref[b * n])) for b in range(B)]
    new = eng.generate(ids, *px, logprobs=True, top_logprobs=3, speculate=k, speculate_selection="any", lookup_ids=look, **kw)
    sp = eng.last_speculation
    assert sp is not None and all(len(sp[f]) == B * n for f in ("steps", "tokens", "drafted", "accepted")), sp
    assert np.array_equal(new, ref)
    for got, want in zip(eng.last_generate_logprobs, ref_lp):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (sp["steps"][::n] < MAX_NEW - 1).all()
    ids4, px4 = sc.gen_inputs(4, V)     # 4 x 2 x 8 = 64 rows > 32: not served; 4 x 2 x 4 = 32: served
    kw4 = dict(kw, max_new_tokens=4)
    want = eng.generate(ids4, *px4, **kw4)
    got = eng.generate(ids4, *px4, speculate=7, speculate_selection="any", **kw4)
    assert np.array_equal(got, want) and eng.last_speculation is None
    got = eng.generate(ids4, *px4, speculate=3, speculate_selection="any", **kw4)
    assert np.array_equal(got, want) and eng.last_speculation is not None


class _Streamer:
    def __init__(self):
        self.got = []

    def put(self, v):
        self.got.append(v.clone())

    def end(self):
        pass


def check_streamer(model, k=3, B=2):
    """the concatenated pieces equal the returned ids, stream_every 1 and 3, through the engine callback and model.generate's streamer"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    kw = dict(SAMPLERS["t0.2_k50"], seed=SEED)
    base, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW, **kw)
    for every in (1, 3):
        got = []
        new = eng.generate(ids, *px, max_new_tokens=MAX_NEW, speculate=k, speculate_selection="any", lookup_ids=sc.lookups("corrupted", base, V),
                           on_tokens=lambda first, a: got.append((first, a.copy())), stream_every=every, **kw)
        assert eng.last_speculation is not None and np.array_equal(new, base)
        assert np.array_equal(np.concatenate([a for _, a in got], 1), new)
        assert [f for f, _ in got] == list(np.cumsum([0] + [a.shape[1] for _, a in got[:-1]]))
        s = _Streamer()
        out = model.generate(torch.from_numpy(ids), max_new_tokens=MAX_NEW, eos_token_id=-1, streamer=s, prompt_lookup_num_tokens=k,
                             speculate_selection="any", lookup_ids=sc.lookups("truth", base, V), images=px[0], segs=px[1], depths=px[2],
                             stream_every=every, **kw)
        assert torch.equal(torch.stack(s.got[1:], 1), out[:, ids.shape[1]:]) and np.array_equal(out[:, ids.shape[1]:].numpy(), base)


def check_new_surface(model, B=2):
    """what the tree without the feature fails: the keyword is swallowed by **kwargs there and `speculation` is None"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    t = torch.from_numpy(ids)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=-1, images=px[0], segs=px[1], depths=px[2], do_sample=True, seed=SEED)
    plain = model.generate(t, **kw)
    truth = [list(map(int, r)) for r in plain[:, ids.shape[1]:].numpy()]
    out = model.generate(t, prompt_lookup_num_tokens=3, speculate_selection="any", lookup_ids=truth, return_dict_in_generate=True, **kw)
    assert torch.equal(out.sequences, plain)
    assert out.speculation is not None, "a sampled call with speculate_selection='any' was not served"
    assert (out.speculation["steps"] < out.speculation["tokens"]).all(), out.speculation
    # the default scope is unchanged
    out = model.generate(t, prompt_lookup_num_tokens=3, lookup_ids=truth, return_dict_in_generate=True, **kw)
    assert torch.equal(out.sequences, plain) and out.speculation is None
    out = model.generate(t, prompt_lookup_num_tokens=3, speculate_selection="greedy", lookup_ids=truth, return_dict_in_generate=True, **kw)
    assert torch.equal(out.sequences, plain) and out.speculation is None


def check_not_served(model, B=2):
    """under "any": beams, split / strict precision, a host-loop stopping criterion, processors_on_device=False, a processor set that
    does not fit the device, fan_out=True, B (k + 1) > 32 — the plain call's output, speculation None; another string: ValueError
    before the engine is touched"""
    import pytest

    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    t = torch.from_numpy(ids)
    kw = dict(max_new_tokens=4, eos_token_id=-1, images=px[0], segs=px[1], depths=px[2])
    samp = dict(do_sample=True, temperature=0.8, top_k=20, seed=3)
    base, _ = sc.session_reference(eng, ids, px, max_new_tokens=4)
    look = sc.lookups("truth", base, V)

    class HostCrit:   # no token-id form: the host loop
        def __call__(self, ids_, scores):
            return False

    many = [[3 + i] for i in range(33)]   # more bad words than the device table holds
    cases = [dict(num_beams=2), dict(stopping_criteria=[HostCrit()], **samp), dict(repetition_penalty=1.3, processors_on_device=False),
             dict(bad_words_ids=many, **samp), dict(num_return_sequences=2, fan_out=True, **samp)]
    for extra in cases:
        want = model.generate(t, **kw, **extra)
        got = model.generate(t, prompt_lookup_num_tokens=3, speculate_selection="any", lookup_ids=look, return_dict_in_generate=True, **kw, **extra)
        assert torch.equal(got.sequences, want), f"not served {list(extra)}: the ids differ"
        assert got.speculation is None and eng.last_speculation is None, f"not served {list(extra)}: speculation reported"
    s = dict(do_sample=True, temperature=0.8, top_k=20, seed=3)
    for mode in ("split", "strict"):
        eng.set_precision(mode)
        try:
            want = eng.generate(ids, *px, max_new_tokens=4, **s)
            got = eng.generate(ids, *px, max_new_tokens=4, speculate=3, speculate_selection="any", lookup_ids=look, **s)
            assert np.array_equal(got, want) and eng.last_speculation is None, mode
        finally:
            eng.set_precision("bf16")
    ids5, px5 = sc.gen_inputs(5, V)     # 5 x 8 rows > 32
    want = eng.generate(ids5, *px5, max_new_tokens=4, **s)
    got = eng.generate(ids5, *px5, max_new_tokens=4, speculate=7, speculate_selection="any", **s)
    assert np.array_equal(got, want) and eng.last_speculation is None
    got = eng.generate(ids5, *px5, max_new_tokens=4, speculate=5, speculate_selection="any", **s)   # 5 x 6 = 30 rows: served
    assert np.array_equal(got, want) and eng.last_speculation is not None
    n0 = model._generation
    for bad in ("sampled", "", "ANY", None):
        with pytest.raises(ValueError):
            model.generate(t, prompt_lookup_num_tokens=3, speculate_selection=bad, **kw)
        with pytest.raises(ValueError):
            eng.generate(ids, *px, max_new_tokens=4, speculate=3, speculate_selection=bad)
    assert model._generation == n0
    with pytest.raises(ValueError):   # also without a speculation request
        model.generate(t, speculate_selection="other", **kw)
    assert model._generation == n0
    assert eng.lib.vc_request_speculation_selection(eng._model, 1) != 0, "the selection was accepted without a pending request"
    assert np.array_equal(eng.generate(ids, *px, max_new_tokens=4), base)


def check_captures(model, B=2):
    """a second identical served call replays; a call of another form — greedy-only speculation behind a sampled one, a processor set
    added — captures exactly one new step; a plain sampled generate behind a served one returns what it returned before"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = sc.gen_inputs(B, V)
    kw = dict(SAMPLERS["t0.2_k50"], seed=SEED, max_new_tokens=MAX_NEW)
    plain = eng.generate(ids, *px, **kw)
    truth, _ = sc.session_reference(eng, ids, px, **kw)
    assert np.array_equal(plain, truth)
    look = sc.lookups("corrupted", truth, V)
    spec = dict(speculate=3, speculate_selection="any", lookup_ids=look)
    a = eng.generate(ids, *px, **kw, **spec)
    c0 = eng.step_captures()
    b = eng.generate(ids, *px, **kw, **spec)
    assert eng.step_captures() == c0, "a second identical served call captured again"
    assert np.array_equal(a, truth) and np.array_equal(b, truth)
    c = eng.generate(ids, *px, **dict(kw, seed=SEED + 1), **spec)     # another seed, other parameters: the records, not the step
    eng.generate(ids, *px, **dict(kw, temperature=0.7, top_k=0, top_p=0.8), **spec)
    g_any = eng.generate(ids, *px, max_new_tokens=MAX_NEW, **spec)   # a greedy call under "any" takes the same step
    assert eng.step_captures() == c0, "another seed / sampler / a greedy call under 'any' captured again"
    greedy, _ = sc.session_reference(eng, ids, px, max_new_tokens=MAX_NEW)
    assert np.array_equal(g_any, greedy)
    c1 = eng.step_captures()
    g = eng.generate(ids, *px, max_new_tokens=MAX_NEW, speculate=3, lookup_ids=look)    # greedy-only speculation: the argmax step
    assert eng.step_captures() == c1 + 1 and np.array_equal(g, greedy), "greedy-only speculation behind a served sampled call must capture exactly one step"
    a = eng.generate(ids, *px, **kw, **spec)
    assert eng.step_captures() == c1 + 2 and np.array_equal(a, truth)
    proc = lp.make(1.3)
    own, _ = sc.session_reference(eng, ids, px, processors=proc, **kw)
    c2 = eng.step_captures()
    p = eng.generate(ids, *px, processors=proc, **kw, **spec)
    assert eng.step_captures() == c2 + 1 and np.array_equal(p, own), "a processor set added must capture exactly one step"
    p = eng.generate(ids, *px, processors=proc, **kw, **spec)
    assert eng.step_captures() == c2 + 1 and np.array_equal(p, own)
    assert np.array_equal(eng.generate(ids, *px, **kw), plain), "a plain sampled generate behind a served one differs"


def check_true_dims(B, k=7, n_new=24, K=3):
    """7b dims, 2 decoder layers, the image prompt (S = 1216): a sampled call with a repetition penalty and log-probs, the truth as
    lookup_ids — ids and log-probs equal the plain session loop's, in fewer steps than tokens"""
    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine

    cfg = vcfg.vicuna_7b("vcoder_ds")
    cfg.num_hidden_layers = 2
    cfg.vit_num_layers = 3
    eng = HipEngine(cfg)
    try:
        eng.load_synthetic(21)
        eng.finalize()
        ids = np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b) for b in range(B)])
        px = synth.synth_batch(B, 336)
        kw = dict(max_new_tokens=n_new, logprobs=True, top_logprobs=K, do_sample=True, temperature=0.2, top_k=50, seed=SEED, processors=lp.make(1.1))
        ref = eng.generate(ids, *px, **kw)
        ref_lp = eng.last_generate_logprobs
        assert int(eng.lib.vc_last_spliced_len(eng._model)) == 1216 and eng.last_speculation is None
        new = eng.generate(ids, *px, speculate=k, speculate_selection="any", lookup_ids=[list(map(int, r)) for r in ref], **kw)
        sp = eng.last_speculation
        assert sp is not None, "the request was not served at 7b dims"
        assert np.array_equal(new, ref), f"7b dims B {B}: ids differ\n{new}\n{ref}"
        for got, want, name in zip(eng.last_generate_logprobs, ref_lp, ("token_logprobs", "top_logprobs", "top_ids")):
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"7b dims B {B}: {name} differ"
        assert (sp["steps"] < n_new - 1).all() and (sp["tokens"] == n_new - 1).all(), sp
        print(f"7b dims B {B} k {k} sampled + repetition penalty: {n_new} tokens in {sp['steps'].tolist()} verify steps, accepted "
              f"{sp['accepted'].tolist()} of {sp['drafted'].tolist()}")
    finally:
        eng.close()
