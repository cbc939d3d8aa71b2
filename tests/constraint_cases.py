"""Constrained decoding (vcoder_amd/constraints.py TokenAutomaton, vck_logits_process_constrained, vc_request_constraint,
generate(constraint=, prefix_allowed_tokens_fn=)): the checks shared by the CPU-emulator tests (tests/test_constraint_emu.py) and the
`-m gpu` tests (tests/test_gpu_constraint.py).

The kernel's reference is logits_processor_cases.ref_process (the numpy float32 restatement of the processors) followed by the mask
of the row's automaton state; every comparison is bit equality.  End to end the reference is the host loop under
`constraint.as_prefix_allowed_tokens_fn(T)`, the automaton's definition."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import torch

import kernel_cases as kc
import logits_processor_cases as pc
import logprob_cases as lc
from score_cases import KERNEL_BAR
from vcoder_amd import _lib as vlib
from vcoder_amd import logits_processors as lp
from vcoder_amd.constraints import TokenAutomaton

# ---- kernel ------------------------------------------------------------------------------------------------------------------
# (rows, V, ldl, shift): the shapes of the processor kernel's tests, one whose odd stride and shift put every row at another
# 4-byte offset (the 16-byte head / body / tail split of the mask), and one vocabulary above the 262144 ids the kernel's LDS bitmap
# holds (the searched path)
KERNEL_SHAPES_EMU = pc.KERNEL_SHAPES_EMU + [(4, 37, 39, 3), (1, 262147, 262152, 1)]
KERNEL_SHAPES_GPU = pc.KERNEL_SHAPES_GPU + [(4, 37, 39, 3), (1, 262147, 262152, 1)]
RS = dict(pc.RS, CN_ON=110, CN_STATE=111, CN_POS=112)   # csrc/kernels.h RowStateField
CHAIN = 6   # states 0 .. CHAIN of the kernel automaton form a chain the lagging rows walk


def kernel_automaton(V, rng):
    """-> (TokenAutomaton, {name: state}, chain ids): states 0 .. CHAIN: state i goes to i + 1 under chain[i] and allows chain[i] + 1
    too (a dead end); behind them the named states of the mask tests"""
    chain = [int(t) for t in rng.choice(np.arange(2, V - 2), size=CHAIN, replace=False)]
    edges, dflt, names = [], [], {}
    for i in range(CHAIN):
        edges.append({chain[i]: i + 1, chain[i] + 1: -1})
        dflt.append(-1)
    edges.append({1: CHAIN, V - 2: CHAIN})   # the chain's end: loops
    dflt.append(-1)

    def add(name, e, d=-1):
        names[name] = len(edges)
        edges.append(dict(e))
        dflt.append(d if d != "self" else len(edges) - 1)

    add("edge_0", {0: 0})
    add("edge_V-1", {V - 1: 0})
    # ids round every boundary a chunk of four can have, at the front, in the middle and at the end of the row, for any row offset
    mid = (V // 2) & ~3
    straddle = set(range(1, 9)) | set(range(mid - 1, mid + 8, 2)) | set(range(V - 9, V - 1, 1)) - {V - 4}
    add("straddle", {t: 0 for t in straddle if 0 <= t < V})
    add("every_id", {t: 0 for t in range(V)})
    add("outside", {-5: 0, -1: 0, 3: 0, V: 0, V + 7: 0})
    add("free_redirect", {2: 0, V - 3: -1}, "self")
    add("random_third", {int(t): 0 for t in rng.choice(V, size=max(V // 3, 1), replace=False)})
    add("combined", {3: 0, 7: 0, 11: 0, V - 1: 0})   # with the processors of _combined_row: 3 penalised + allowed, 5 penalised + disallowed
    off, tok, nxt = [0], [], []
    for e in edges:
        for t in sorted(e):
            tok.append(t)
            nxt.append(e[t])
        off.append(len(tok))
    return TokenAutomaton.from_edges(np.asarray(off), np.asarray(tok), np.asarray(nxt), np.asarray(dflt)), names, chain


def mask_state(a, row, state, V):
    """the numpy restatement of phase 4: `row` [V] under `state`"""
    if 0 <= state < a.num_states and a.default_next[state] >= 0:
        return row
    out = np.full_like(row, -np.inf)
    ok = [t for t in a.allowed(state) if 0 <= t < V]
    out[ok] = row[ok]
    return out


def _kernel_rows(a, names, chain, V, rng):
    """the row scenarios: dicts of the processor settings of pc.check_logits_process's rows plus on / state / pos (the stored
    automaton state and the ids it has consumed), active, finished"""
    rnd = lambda n: [int(t) for t in rng.randint(0, V, size=n)]
    R = []

    def add(name, state=0, pos=None, gen=(), on=1, active=1, finished=0, **proc):
        gen = list(gen)
        R.append(dict(dict(name=name, prompt=rnd(4), gen=gen, penalty=1.0, ngram=0, bad=[], min_new=0, eos=-1, eos_extra=[], on=on,
                           state=state, pos=len(gen) if pos is None else pos, active=active, finished=finished), **proc))

    for n, s in names.items():
        if n != "combined":
            add(n, state=s, gen=rnd(2))
    add("dead", state=-1, gen=rnd(1))
    add("state_outside_table", state=a.num_states + 3, gen=rnd(1))
    add("step0", state=0)
    for lag in (0, 1, 3):   # the stored state lags RS_STEP: the same row, the same state afterwards
        for step in (3, CHAIN):
            add(f"lag{lag}_step{step}", state=step - lag, pos=step - lag, gen=chain[:step])
    add("walks_off", state=0, pos=0, gen=[chain[0], chain[1] + 1, 5])   # an id with an edge to the dead state, then anything
    add("walks_disallowed", state=1, pos=1, gen=[chain[0], chain[2]])   # an id the state does not allow: default_next = dead
    add("off", state=names["edge_0"], gen=rnd(2), on=0)
    add("finished", state=names["edge_0"], gen=rnd(2), finished=1)
    add("inactive", state=names["edge_0"], gen=rnd(2), active=0)
    # every other processor on: 3 and 5 are penalised (history) — 3 is allowed and keeps the penalised bits, 5 is not and ends -inf;
    # 7 is allowed and a bad word, 11 allowed and the EOS under min_new_tokens: -inf; V - 1 allowed and untouched
    add("combined", state=names["combined"], prompt=[3, 5, 9, 13], gen=[9, 13, 9], penalty=1.3, ngram=2, bad=[[7]], min_new=5, eos=11,
        eos_extra=[4])
    return R


def check_constrained_kernel(be, rows, V, ldl, shift, seed=0):
    rng = np.random.RandomState(seed + rows * 11 + V)
    a, names, chain = kernel_automaton(V, rng)
    scen = _kernel_rows(a, names, chain, V, rng)
    d_tab = [be.i32(np.ascontiguousarray(t)) for t in a.tables()]
    null = None
    seen = set()
    for launch in range(-(-len(scen) // rows)):
        use = [scen[(launch * rows + r) % len(scen)] for r in range(rows)]
        raw = np.full(shift + rows * ldl + 3, np.nan, dtype=np.float32)
        rec = kc.make_rows(rows)
        table, prompt, gen = [], [], []
        for r, s in enumerate(use):
            raw[shift + r * ldl: shift + r * ldl + V] = (rng.randn(V) * 3).astype(np.float32)
            table += s["bad"]
            rec[r, RS["ACTIVE"]] = s["active"]
            rec[r, RS["FINISHED"]] = s["finished"]
            rec[r, RS["STEP"]] = len(s["gen"])
            rec[r, RS["MAXNEW"]] = len(s["gen"]) + 2
            rec[r, RS["EOS"]] = s["eos"]
            rec[r, RS["OUT_OFF"]] = len(gen)
            rec[r, RS["LP_PENALTY"]] = kc._f32_bits(s["penalty"])
            rec[r, RS["LP_NGRAM"]] = s["ngram"]
            rec[r, RS["LP_MINNEW"]] = s["min_new"]
            rec[r, RS["LP_HIST_OFF"]] = len(prompt)
            rec[r, RS["LP_HIST_LEN"]] = len(s["prompt"])
            rec[r, RS["LP_NBAD"]] = len(table) if s["bad"] else 0
            rec[r, RS["LP_NEOS"]] = len(s["eos_extra"])
            rec[r, RS["LP_EOS"]: RS["LP_EOS"] + len(s["eos_extra"])] = s["eos_extra"]
            rec[r, RS["CN_ON"]] = s["on"]
            rec[r, RS["CN_STATE"]] = s["state"]
            rec[r, RS["CN_POS"]] = s["pos"]
            prompt += s["prompt"]
            gen += s["gen"] + [V + 5, -7]   # what stands behind the ids generated so far is never read
        tab = np.zeros((pc.MAX_BAD, 1 + pc.MAX_BAD_LEN), dtype=np.int32)
        for q, w in enumerate(table):
            tab[q, 0] = len(w)
            tab[q, 1: 1 + len(w)] = w
        d_raw = be.f32(raw)
        d_prompt, d_gen, d_bad = be.i32(np.asarray(prompt + [0], np.int32)), be.i32(np.asarray(gen, np.int32)), be.i32(tab)
        # the launch without tables (both entries): the bytes vck_logits_process writes, and records nobody wrote
        d_plain, d_rec0 = be.f32(np.full_like(raw, np.nan)), be.i32(rec)
        kc._call(be, "vck_logits_process", d_raw[shift:], ldl, d_plain[shift:], ldl, d_rec0, d_prompt, d_gen, d_bad, rows, V)
        plain = be.host_f32(d_plain)
        d_off, d_rec1 = be.f32(np.full_like(raw, np.nan)), be.i32(rec)
        kc._call(be, "vck_logits_process_constrained", d_raw[shift:], ldl, d_off[shift:], ldl, d_rec1, d_prompt, d_gen, d_bad, null, null,
                 null, null, 0, rows, V)
        assert np.array_equal(be.host_f32(d_off).view(np.int32), plain.view(np.int32)), "tables off: not the bytes of vck_logits_process"
        assert np.array_equal(be.host_i32(d_rec1), rec), "tables off: the records were written"
        d_out, d_rec = be.f32(np.full_like(raw, np.nan)), be.i32(rec)
        kc._call(be, "vck_logits_process_constrained", d_raw[shift:], ldl, d_out[shift:], ldl, d_rec, d_prompt, d_gen, d_bad, *d_tab,
                 a.num_states, rows, V)
        got, rec_after = be.host_f32(d_out), be.host_i32(d_rec).reshape(rows, -1)
        assert np.array_equal(be.host_f32(d_raw).view(np.int32), raw.view(np.int32)), "the raw rows were written"
        assert np.isnan(got[:shift]).all() and np.isnan(got[shift + rows * ldl:]).all(), "wrote in front of the first / behind the last row"
        for r, s in enumerate(use):
            what = f"constrained rows {rows} V {V} ldl {ldl} shift {shift} launch {launch} row {r} ({s['name']})"
            seen.add(s["name"])
            row = got[shift + r * ldl: shift + (r + 1) * ldl]
            assert np.isnan(row[V:]).all(), f"{what}: pad columns written"
            v = raw[shift + r * ldl: shift + r * ldl + V]
            words = [w for w in table[:int(rec[r, RS["LP_NBAD"]])]]
            step = len(s["gen"])
            ref = pc.ref_process(v, s["prompt"] + s["gen"], s["penalty"], s["ngram"], words, s["min_new"], step, [s["eos"]] + s["eos_extra"])
            want_rec = rec[r].copy()
            if not s["active"]:
                ref = np.full(V, np.nan, dtype=np.float32)   # an inactive row is not written at all
            elif s["on"] and not s["finished"]:
                st = a.walk(s["gen"][s["pos"]:], s["state"]) if 0 <= s["state"] < a.num_states else -1
                assert st == (a.walk(s["gen"]) if s["name"].startswith(("lag", "walks")) else st), "the scenario's stored state is no cache"
                want_rec[RS["CN_STATE"]], want_rec[RS["CN_POS"]] = st, step
                masked = mask_state(a, ref, st, V)
                if s["name"] == "combined":   # the scenario shows what it is there to show
                    assert masked[3] == np.float32(v[3] * np.float32(1.3) if v[3] < 0 else v[3] / np.float32(1.3)) and masked[V - 1] == v[V - 1]
                    assert all(masked[t] == -np.inf for t in (5, 7, 11)) and ref[5] != -np.inf and ref[5] != v[5]
                if s["name"] in ("every_id", "free_redirect"):
                    assert np.array_equal(masked.view(np.int32), ref.view(np.int32))
                if s["name"] in ("dead", "state_outside_table", "walks_off", "walks_disallowed"):
                    assert np.isneginf(masked).all()
                if s["name"] in ("edge_0", "edge_V-1", "outside"):
                    assert (~np.isneginf(masked)).sum() <= 1
                ref = masked
            else:
                assert np.array_equal(row[:V].view(np.int32), plain[shift + r * ldl: shift + r * ldl + V].view(np.int32)), f"{what}: differs from the launch without tables"
            bad = np.nonzero(row[:V].view(np.int32) != ref.view(np.int32))[0]
            assert bad.size == 0, f"{what}: ids {bad[:8]}: got {row[bad[:8]]}, restatement {ref[bad[:8]]}, raw {v[bad[:8]]}"
            assert np.array_equal(rec_after[r], want_rec), f"{what}: record {np.nonzero(rec_after[r] != want_rec)[0]} after the launch"
    assert seen == {s["name"] for s in scen}


# ---- host semantics ------------------------------------------------------------------------------------------------------------
def check_apply_prefix_constraint_against_hf(seed=0, V=53, trials=40):
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor

    rng = np.random.RandomState(seed)
    compared = 0
    for trial in range(trials):
        nb = int(rng.choice([1, 2, 3]))
        B, L = int(rng.randint(1, 4)), int(rng.randint(1, 7))
        hist = torch.from_numpy(rng.randint(0, V, size=(B * nb, L)).astype(np.int64))
        scores = torch.from_numpy((rng.randn(B * nb, V) * 3).astype(np.float32))
        scores[0, int(rng.randint(0, V))] = float("-inf")
        table = {}

        def fn(b, ids):
            key = (int(b), tuple(int(t) for t in ids))
            if key not in table:
                n = int(rng.choice([0, 1, 5, 5, 9, V, V]))
                table[key] = sorted(int(t) for t in rng.choice(V, size=n, replace=False))
            return table[key]

        got = lp.apply_prefix_constraint(fn, hist, scores, nb)
        empty = [r for r in range(B * nb) if not fn(r // nb, hist[r])]
        assert all(bool(torch.isneginf(got[r]).all()) for r in empty), "an empty list leaves the row all -inf (4.31)"
        try:
            want = PrefixConstrainedLogitsProcessor(fn, nb)(hist, scores.clone())
        except ValueError:   # later releases refuse an empty list, where 4.31 returns the all -inf row
            assert empty
            continue
        assert torch.equal(got, want), f"trial {trial}"
        compared += 1
    assert compared >= trials // 4
    skip = torch.tensor([True] + [False] * (B * nb - 1))
    got = lp.apply_prefix_constraint(lambda b, ids: [], hist, scores, nb, skip=skip)
    assert torch.equal(got[0], scores[0]) and bool(torch.isneginf(got[1:]).all())


ALPHABET = list(range(20, 32))   # 12 ids


def _language(a, max_len=6):
    """brute force over the alphabet: (complete answers: sequences that reach a final state with their last id, live prefixes)"""
    done, live = set(), {()}
    front = [((), 0)]
    for _ in range(max_len):
        nxt = []
        for seq, st in front:
            for t in ALPHABET:
                s2 = a.step(st, t)
                if t not in a.allowed(st):
                    assert a.walk(seq + (t,)) == -1
                    continue
                assert s2 >= 0, "the builders' automata have no allowed id that leads to the dead state"
                live.add(seq + (t,))
                if s2 in a.final and st not in a.final:
                    done.add(seq + (t,))
                if s2 not in a.final:
                    nxt.append((seq + (t,), s2))
        front = nxt
    return done, live


def _prefixes(words, max_len):
    return {w[:n] for w in words for n in range(min(len(w), max_len) + 1)}


def check_builders(max_len=6):
    a_, b_, c_, d_, e_, f_, g_, h_ = ALPHABET[:8]
    end = [ALPHABET[10], ALPHABET[11]]
    # from_sequences: shared prefixes, one sequence a prefix of another, duplicates
    seqs = [[a_, b_], [a_, b_, c_], [a_, d_], [e_], [e_], [f_, f_, f_, f_, f_], [g_, a_, b_, c_, d_, e_]]
    a = TokenAutomaton.from_sequences(seqs, end)
    want = {tuple(q) + (e,) for q in seqs for e in end}
    done, live = _language(a, max_len)
    assert done == {w for w in want if len(w) <= max_len}, "from_sequences: the accepted language"
    assert live == _prefixes(want, max_len), "from_sequences: the live prefixes"
    assert a.walk(list(next(iter(want)))) in a.final and a.walk([a_, a_]) == -1 and a.allowed(-1) == []
    # from_list: brute force of prefix item (sep item)* term end under min / max items
    items, sep, term, pre = [[a_], [b_, c_], [b_, d_], [b_]], [e_], [f_], [g_]
    for mn, mx, sep_, term_, pre_ in ((1, None, sep, term, pre), (2, 3, sep, term, pre), (1, 2, [e_, h_], [], []), (2, None, sep, [f_, h_], [])):
        a = TokenAutomaton.from_list(pre_, items, sep_, term_, end, min_items=mn, max_items=mx)
        want = set()
        for n in range(mn, (mx or max_len) + 1):
            for pick in itertools.product(items, repeat=n):
                body = list(pre_)
                for j, it in enumerate(pick):
                    body += (sep_ if j else []) + it
                if len(body) + len(term_) + 1 <= max_len:
                    want |= {tuple(body + term_) + (e,) for e in end}
        done, live = _language(a, max_len)
        assert done == want and want, f"from_list min {mn} max {mx}: accepts {sorted(done ^ want)[:4]} otherwise"
    fn = a.as_prefix_allowed_tokens_fn(2)
    assert fn(0, torch.tensor([7, 7])) == a.allowed(0) and fn(1, torch.tensor([7, 7, a_, a_])) == []
    # nondeterminism: the separator / terminator first id continues a longer item at an item end
    for kw in (dict(separator=[c_]), dict(terminator=[d_]), dict(terminator=[], end_ids=[c_]), dict(terminator=[e_])):
        args = dict(prefix=[], items=items, separator=sep, terminator=term, end_ids=end)
        args.update(kw)
        try:
            TokenAutomaton.from_list(**args)
            raise AssertionError(f"from_list({kw}) is nondeterministic and was accepted")
        except ValueError as e:
            assert "nondeterministic" in str(e) and any(str(t) in str(e) for t in (c_, d_, e_)), e
    try:
        TokenAutomaton.from_sequences([[a_], [a_, end[0]]], end)
        raise AssertionError("from_sequences: an end id continues a longer sequence")
    except ValueError as e:
        assert "nondeterministic" in str(e)
    # validation of raw tables
    ok = dict(state_off=[0, 2, 3], edge_tok=[1, 4, 2], edge_next=[1, -1, 0], default_next=[-1, 1])
    TokenAutomaton.from_edges(**ok)
    big = TokenAutomaton.from_edges(np.arange(65537), np.zeros(65536, np.int64), np.zeros(65536, np.int64), np.full(65536, -1))
    assert big.num_states == 65536
    for bad in (dict(edge_tok=[4, 1, 2]), dict(edge_tok=[1, 1, 2]), dict(edge_next=[2, -1, 0]), dict(edge_next=[1, -2, 0]),
                dict(default_next=[-1, 2]), dict(state_off=[0, 3, 2]), dict(state_off=[0, 2]), dict(state_off=[1, 2, 3]),
                dict(state_off=[0, 3, 3], default_next=[-1, -1]),                      # state 1: reachable, allows nothing
                dict(state_off=np.arange(65538), edge_tok=np.zeros(65537, np.int64), edge_next=np.zeros(65537, np.int64),
                     default_next=np.full(65537, -1)),                                 # S > 65536
                dict(state_off=[0, (1 << 20) + 1], edge_tok=np.arange((1 << 20) + 1), edge_next=np.zeros((1 << 20) + 1, np.int64),
                     default_next=[-1])):                                              # E > 1 << 20
        try:
            TokenAutomaton.from_edges(**dict(ok, **bad))
            raise AssertionError(f"from_edges accepted {list(bad)}")
        except ValueError:
            pass
    TokenAutomaton.from_edges([0, 3, 3], [1, 2, 4], [0, 0, 0], [-1, -1])   # state 1 allows nothing, but nothing leads there


# ---- engine and model ------------------------------------------------------------------------------------------------------------
N_NEW = 8
inputs_for = pc.inputs_for
_models = {}


def model_for(variant, lib=None, operands="bf16", seed=42):
    """one model per (variant, library) for the tests of this feature alone, released by close_models() when a module is through:
    the sessions other modules share keep the buffers, the captured steps and the device addresses they would have without these
    tests (some of them assert on re-captures, which follow the addresses the allocator hands back)"""
    import e2e_cases
    import score_cases as sc

    key = (variant, id(lib), operands)
    if key not in _models:
        kw = {"_lib_override": lib} if lib is not None else {}
        m = sc._CLASSES[variant](e2e_cases.tiny_cfg(variant), device="cuda", operands=operands, **kw)
        m.engine.load_synthetic(seed)
        m.finalize_weights()
        _models[key] = m
    return _models[key]


def close_models():
    for m in _models.values():
        m.engine.close()
    _models.clear()


def _gen(model, ids, px, **kw):
    kw.setdefault("max_new_tokens", N_NEW)
    kw.setdefault("eos_token_id", -1)
    return model.generate(torch.from_numpy(ids), **px, **kw)


def alphabet_from(plain_new, V):
    """16 ids the unconstrained call never emits, spread over the vocabulary"""
    used = {int(t) for t in plain_new.reshape(-1)}
    free = [t for t in range(7, V) if t not in used]
    assert len(free) >= 16
    return free[:: max(len(free) // 16, 1)][:16]


def automata_from(plain_new, V):
    """the automata of the end-to-end cases, over ids the unconstrained call `plain_new` [B, n] never emits — so it rejects every row
    of that call.  -> {"list": a class list, "one_of": one of a few strings, "free_then": two tokens of free text, then the list},
    the end id"""
    A = alphabet_from(plain_new, V)
    items = [[A[0]], [A[0], A[3]], [A[1], A[2]], [A[1], A[3]], [A[4], A[5], A[6]], [A[4]], [A[7], A[0]], [A[7], A[2]], [A[7], A[5]]]
    end = A[10]
    lst = TokenAutomaton.from_list([A[11]], items, [A[8]], [A[9]], [end], min_items=2, max_items=3)
    one = TokenAutomaton.from_sequences([[A[0], A[1], A[2]], [A[0], A[3]], [A[5], A[5], A[5], A[5]], [A[12], A[13], A[14], A[15], A[0], A[1]]], [end])
    # two tokens of free text in front of the list: states 0, 1 free, then `lst` shifted by two
    off, tok, nxt, dflt = lst.tables()
    ft = TokenAutomaton.from_edges(np.concatenate([[0, 0], off]), tok, np.where(nxt >= 0, nxt + 2, nxt), np.concatenate([[1, 2], dflt]))
    # an open list whose item ends allow the separator or the end id: the processors can ban one of the two without a dead end
    opn = TokenAutomaton.from_list([A[11]], items, [A[8]], [], [end])
    return {"list": lst, "one_of": one, "free_then": ft, "open_list": opn}, end


SAMPLE = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=11)


def check_device_vs_host(model, mode, B, sample=False):
    """the device loop under constraint=a returns what the host loop returns under a.as_prefix_allowed_tokens_fn(T, V); every row is
    accepted by a.walk; the call without the constraint yields rows the automaton rejects (which is what fails on an engine that
    swallows the argument).  Sampled: the device sampler's stream is not torch.multinomial's, so the sampled device call is compared
    with the host loop at top_k = 1 (one candidate survives the warpers: both samplers must pick it) and checked for acceptance and
    repeatability at the usual settings."""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T, V = ids.shape[1], model.config.vocab_size
        skw = dict(SAMPLE, top_k=1) if sample else {}
        plain = _gen(model, ids, px, **skw)
        autos, end = automata_from(plain[:, T:].numpy(), V)
        for name, a in autos.items():
            if name == "open_list":
                continue
            assert all(a.walk(row) == -1 for row in plain[:, T:].tolist()), f"precondition ({name}): an unconstrained row is accepted"
            for kw in (dict(eos_token_id=-1), dict(eos_token_id=end, pad_token_id=0)):
                dev = _gen(model, ids, px, constraint=a, **skw, **kw)
                host = _gen(model, ids, px, prefix_allowed_tokens_fn=a.as_prefix_allowed_tokens_fn(T, V), **skw, **kw)
                off = _gen(model, ids, px, constraint=a, processors_on_device=False, **skw, **kw)
                print(f"[{mode}] B {B} sample {sample} {name} {kw}: plain {plain[:, T:].tolist()} device {dev[:, T:].tolist()}")
                assert torch.equal(dev, host), f"[{mode}] B {B} {name}: device loop {dev[:, T:].tolist()}, host loop {host[:, T:].tolist()}"
                assert torch.equal(off, host), "constraint= on the host loop differs from its own callable"
                for row in dev[:, T:].tolist():
                    cut = row[: row.index(end) + 1] if kw["eos_token_id"] == end and end in row else row
                    assert a.walk(cut) >= 0, f"[{mode}] B {B} {name}: the automaton rejects {row}"
                    assert all(t == 0 for t in row[len(cut):])
            if sample:
                one = _gen(model, ids, px, constraint=a, **SAMPLE)
                assert torch.equal(one, _gen(model, ids, px, constraint=a, **SAMPLE)), "a sampled call does not repeat under its seed"
                assert all(a.walk(row) >= 0 for row in one[:, T:].tolist()), f"[{mode}] B {B} {name}: a sampled row is rejected"
    finally:
        eng.set_precision("bf16")


def check_with_processors(model, mode, B):
    """all five processors and the constraint: device loop = host loop; the ids obey both"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T, V = ids.shape[1], model.config.vocab_size
        plain = _gen(model, ids, px)
        autos, end = automata_from(plain[:, T:].numpy(), V)
        a = autos["open_list"]
        alone = _gen(model, ids, px, constraint=a, eos_token_id=end, pad_token_id=0)
        new = alone[:, T:].numpy()
        # the first id of the item row 0 picks, and the one-id item behind a separator, are bad words: other items stay allowed; the
        # end id is banned for 6 tokens, where the open list goes on with a separator
        A = alphabet_from(plain[:, T:].numpy(), V)
        words = [[int(new[0, 1])], [A[8], A[0]]]
        kw = dict(repetition_penalty=pc.REP_PENALTY, no_repeat_ngram_size=4, bad_words_ids=words, min_new_tokens=6, min_length=T + 4,
                  eos_token_id=end, pad_token_id=0)
        dev = _gen(model, ids, px, constraint=a, **kw)
        host = _gen(model, ids, px, prefix_allowed_tokens_fn=a.as_prefix_allowed_tokens_fn(T, V), **kw)
        print(f"[{mode}] B {B} all five + list: alone {new.tolist()} device {dev[:, T:].tolist()}")
        assert torch.equal(dev, host), f"[{mode}] B {B}: device loop {dev[:, T:].tolist()}, host loop {host[:, T:].tolist()}"
        assert not torch.equal(dev[:, :alone.shape[1]], alone[:, :dev.shape[1]]), "the processors change nothing: the case shows nothing"
        pc.assert_properties(f"[{mode}] B {B}", ids, dev[:, T:].numpy(), 4, words, 6, [end])
        for row in dev[:, T:].tolist():
            assert a.walk(row[: row.index(end) + 1] if end in row else row) >= 0
    finally:
        eng.set_precision("bf16")


def check_with_logprobs(model, mode, B):
    """the ids are those of the constrained call; the log-probs are those of the RAW rows: equal (bits) to the unconstrained call's
    wherever the ids in front of the step agree, and to the host loop's ids"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T, V = ids.shape[1], model.config.vocab_size
        base = _gen(model, ids, px, output_logprobs=True, top_logprobs=5)
        autos, end = automata_from(base.sequences[:, T:].numpy(), V)
        for name in ("free_then", "list"):
            a = autos[name]
            want = _gen(model, ids, px, constraint=a)
            out = _gen(model, ids, px, constraint=a, output_logprobs=True, top_logprobs=5)
            assert torch.equal(out.sequences, want), "the ids change with the log-prob request"
            host = _gen(model, ids, px, prefix_allowed_tokens_fn=a.as_prefix_allowed_tokens_fn(T, V), output_logprobs=True, top_logprobs=5)
            assert torch.equal(host.sequences, want) and torch.equal(host.top_token_ids, out.top_token_ids)
            # (the host loop's log-probs are torch's log_softmax, the device's its own kernel: the bar of the processor tests)
            assert float((host.token_logprobs - out.token_logprobs).abs().max()) < 2 * KERNEL_BAR
            new, ref = out.sequences[:, T:].numpy(), base.sequences[:, T:].numpy()
            agree_total = 0
            for b in range(B):
                n = next((j for j in range(new.shape[1]) if new[b, j] != ref[b, j]), new.shape[1])   # ids agree in front of step n
                agree_total += n
                bits = lambda t: t.numpy().view(np.int32)
                assert np.array_equal(bits(out.token_logprobs[b, :n]), bits(base.token_logprobs[b, :n])), f"{name} row {b}: token log-probs"
                assert np.array_equal(bits(out.top_logprobs[b, :n + 1]), bits(base.top_logprobs[b, :n + 1])), f"{name} row {b}: top log-probs"
                assert torch.equal(out.top_token_ids[b, :n + 1], base.top_token_ids[b, :n + 1])
                if n < new.shape[1]:   # the constrained token is scored by the raw row: what the unconstrained call's row gives it
                    assert out.token_logprobs[b, n] <= base.token_logprobs[b, n], "the constraint picked a likelier token than the argmax"
            assert name != "free_then" or agree_total >= 2 * B, "two tokens of free text agree with the unconstrained call"
    finally:
        eng.set_precision("bf16")


class _HostOnly:
    """a stopping criterion that never stops and needs host code: the call takes the host loop"""

    def __call__(self, ids, scores):
        return False


def check_stops_stream_fanout(model, B=2):
    """stop sequences, a streamer, a host-only stopping criterion and num_return_sequences = 2 in both forms, each with the
    constraint on the device loop"""
    eng = model.engine
    ids, px = inputs_for(B)
    T, V = ids.shape[1], model.config.vocab_size
    plain = _gen(model, ids, px)
    autos, end = automata_from(plain[:, T:].numpy(), V)
    a = autos["list"]
    full = _gen(model, ids, px, constraint=a)
    new = full[:, T:].numpy()
    # a stop sequence: the second and third token of row 0 — that row is finished behind them (pad), the other rows run on
    stop = [int(new[0, 1]), int(new[0, 2])]
    out = _gen(model, ids, px, constraint=a, pad_token_id=0, stopping_criteria=[lc._DeviceStop([stop])])[:, T:].numpy()
    for b in range(B):
        row = new[b].tolist()
        e = next((j + 2 for j in range(len(row) - 1) if row[j: j + 2] == stop), len(row))
        want = row[:e] + [0] * (out.shape[1] - e)
        assert out[b].tolist() == want[: out.shape[1]], f"stop sequence row {b}: {out[b].tolist()} for {row}"
    assert out.shape[1] <= new.shape[1] and out[0].tolist()[:3] == new[0, :3].tolist()
    # a stopping criterion that needs host code: the host loop under the automaton's callable
    host = _gen(model, ids, px, constraint=a, stopping_criteria=[_HostOnly()])
    assert torch.equal(host, full)

    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got.append(v.clone())

        def end(self):
            pass

    s = Streamer()
    out = _gen(model, ids, px, constraint=a, streamer=s)
    assert torch.equal(out, full) and torch.equal(s.got[0], torch.from_numpy(ids))
    assert torch.equal(torch.stack(s.got[1:], 1), out[:, T:]), "the streamer saw other ids than the call returned"
    # num_return_sequences: rows are independent — the repeated form, the fan-out form and the call on the repeated prompts agree
    rep = np.repeat(np.arange(B), 2)
    px2 = {k: (None if v is None else v[torch.as_tensor(rep)]) for k, v in px.items()}
    want = _gen(model, ids[rep], px2, constraint=a, **SAMPLE)
    for fan in (False, True):
        got = _gen(model, ids, px, constraint=a, num_return_sequences=2, fan_out=fan, **SAMPLE)
        assert eng.last_fanout is not None and eng.last_fanout["shared"] == fan
        assert torch.equal(got, want), f"num_return_sequences=2 fan_out={fan}: {got[:, T:].tolist()} for {want[:, T:].tolist()}"
    assert all(a.walk(row) >= 0 for row in want[:, T:].tolist())


def check_beams(model, B=2):
    """beams: constraint= runs on the host beam loop under its own callable; the device beam ABI refuses a pending constraint"""
    eng = model.engine
    ids, px = inputs_for(B)
    T, V = ids.shape[1], model.config.vocab_size
    plain = _gen(model, ids, px)
    a = automata_from(plain[:, T:].numpy(), V)[0]["one_of"]
    end = automata_from(plain[:, T:].numpy(), V)[1]
    kw = dict(num_beams=2, eos_token_id=end, pad_token_id=0)
    free = _gen(model, ids, px, **kw)
    got = _gen(model, ids, px, constraint=a, **kw)
    want = _gen(model, ids, px, prefix_allowed_tokens_fn=a.as_prefix_allowed_tokens_fn(T, V), **kw)
    assert torch.equal(got, want)
    assert got.shape != free.shape or not torch.equal(got, free), "beam search ignores the constraint"
    for row in got[:, T:].tolist():
        assert end in row and a.walk(row[: row.index(end) + 1]) in a.final, f"beam search: {row} is no complete answer"
    assert torch.equal(_gen(model, ids, px, **kw), free)
    args = (ids, px["images"], px["segs"], px["depths"])
    beam = eng.generate_beam(*args, num_beams=2, max_new_tokens=N_NEW)
    assert eng.lib.vc_request_constraint(eng._model, C.byref(_tables(a)[0])) == 0
    try:
        eng.generate_beam(*args, num_beams=2, max_new_tokens=N_NEW)
        raise AssertionError("vc_generate_beam ran with a vc_request_constraint pending")
    except RuntimeError as e:   # VC_ERR_STATE
        assert "constrained decoding" in str(e)
    again = eng.generate_beam(*args, num_beams=2, max_new_tokens=N_NEW)
    assert all(np.array_equal(x, y) for x, y in zip(beam, again)), "the refused request was not cleared"


def _tables(a):
    keep = [np.ascontiguousarray(t, dtype=np.int32) for t in a.tables()]
    return vlib.TokenAutomatonTables(a.num_states, a.num_edges, *(t.ctypes.data_as(C.c_void_p) for t in keep)), keep


def check_speculation_not_served(model, B=2):
    ids, px = inputs_for(B)
    T, V = ids.shape[1], model.config.vocab_size
    plain = _gen(model, ids, px)
    a = automata_from(plain[:, T:].numpy(), V)[0]["list"]
    want = _gen(model, ids, px, constraint=a)
    for sel in ("greedy", "any"):
        out = _gen(model, ids, px, constraint=a, prompt_lookup_num_tokens=3, speculate_selection=sel, return_dict_in_generate=True)
        assert out.speculation is None and torch.equal(out.sequences, want)
    served = _gen(model, ids, px, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    assert served.speculation is not None and torch.equal(served.sequences, plain), "speculation is still served without a constraint"


def check_no_leak(model, mode, B=2):
    """an unconstrained call behind a constrained one returns what it returned before (the step graphs re-key, the request is
    cleared), also behind a constrained call that failed and behind a request another entry point consumed"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T, V = ids.shape[1], model.config.vocab_size
        plain = _gen(model, ids, px)
        autos, end = automata_from(plain[:, T:].numpy(), V)
        first = _gen(model, ids, px, constraint=autos["list"])
        assert not torch.equal(first, plain)
        assert torch.equal(_gen(model, ids, px), plain), "a plain generate behind a constrained one differs"
        other = _gen(model, ids, px, constraint=autos["one_of"])   # other tables, maybe at the same address
        assert not torch.equal(other, first)
        assert torch.equal(_gen(model, ids, px, constraint=autos["list"]), first)
        rp = _gen(model, ids, px, repetition_penalty=pc.REP_PENALTY)
        assert torch.equal(_gen(model, ids, px, constraint=autos["list"]), first)
        assert torch.equal(_gen(model, ids, px, repetition_penalty=pc.REP_PENALTY), rp), "a processor call behind a constrained one is constrained"
        try:
            _gen(model, ids, px, constraint=autos["list"], max_new_tokens=model.config.max_position_embeddings)
            raise AssertionError("a call over the KV capacity was accepted")
        except (ValueError, RuntimeError, IndexError):
            pass
        assert torch.equal(_gen(model, ids, px), plain), "a constrained call that failed left its request behind"
        args = (ids, px["images"], px["segs"], px["depths"])
        req, keep = _tables(autos["list"])
        assert eng.lib.vc_request_constraint(eng._model, C.byref(req)) == 0
        eng.prefill(*args)
        assert np.array_equal(eng.generate(*args, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a request outlived another entry point"
        assert eng.lib.vc_request_constraint(eng._model, C.byref(req)) == 0
        assert eng.lib.vc_request_constraint(eng._model, None) == 0
        assert np.array_equal(eng.generate(*args, max_new_tokens=N_NEW), plain[:, T:].numpy()), "a cancelled request fired"
        assert eng.lib.vc_request_constraint(eng._model, C.byref(req)) == 0
        assert np.array_equal(eng.generate(*args, max_new_tokens=N_NEW), first[:, T:].numpy()), "a request through the ABI alone does nothing"
        assert np.array_equal(eng.generate(*args, max_new_tokens=N_NEW), plain[:, T:].numpy())
    finally:
        eng.set_precision("bf16")


def check_refusals(model, B=2):
    """argument errors before the engine is touched; bad tables refused by the C entry (VC_ERR_INVALID -> ValueError)"""
    eng = model.engine
    ids, px = inputs_for(B)
    T, V = ids.shape[1], model.config.vocab_size
    plain = _gen(model, ids, px)
    a = automata_from(plain[:, T:].numpy(), V)[0]["list"]
    fn = a.as_prefix_allowed_tokens_fn(T, V)
    calls = eng.step_captures()
    for kw in (dict(constraint=a, prefix_allowed_tokens_fn=fn), dict(constraint=fn), dict(constraint=[[1, 2]]), dict(prefix_allowed_tokens_fn=a),
               dict(constraint=a, prefix_allowed_tokens_fn=fn, num_beams=2)):
        try:
            _gen(model, ids, px, **kw)
            raise AssertionError(f"generate({list(kw)}) was accepted")
        except ValueError:
            pass
    try:
        eng.generate(ids, px["images"], px["segs"], px["depths"], max_new_tokens=N_NEW, constraint=fn)
        raise AssertionError("HipEngine.generate(constraint=<callable>) was accepted")
    except ValueError:
        pass
    assert eng.step_captures() == calls
    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    ok = dict(state_off=i32(0, 2, 3), edge_tok=i32(1, 4, 2), edge_next=i32(1, -1, 0), default_next=i32(-1, 1))
    for bad in (dict(edge_tok=i32(4, 1, 2)), dict(edge_tok=i32(1, 1, 2)), dict(edge_next=i32(2, -1, 0)), dict(edge_next=i32(1, -2, 0)),
                dict(default_next=i32(-1, 2)), dict(default_next=i32(-2, 1)), dict(state_off=i32(0, 3, 2)), dict(state_off=i32(1, 2, 3)),
                dict(state_off=i32(0, 3, 3), default_next=i32(-1, -1))):
        t = dict(ok, **bad)
        raw = TokenAutomaton(t["state_off"], t["edge_tok"], t["edge_next"], t["default_next"])   # (the constructor does not validate)
        try:
            _gen(model, ids, px, constraint=raw)
            raise AssertionError(f"bad tables ({list(bad)}) were accepted")
        except ValueError as e:
            assert "vc_request_constraint" in str(e)
    for S, E in ((0, 0), (65537, 3), (2, -1), (2, (1 << 20) + 1)):
        req = vlib.TokenAutomatonTables(S, E, *(ok[k].ctypes.data_as(C.c_void_p) for k in ("state_off", "edge_tok", "edge_next", "default_next")))
        assert eng.lib.vc_request_constraint(eng._model, C.byref(req)) == -1
    req = vlib.TokenAutomatonTables(2, 3, ok["state_off"].ctypes.data_as(C.c_void_p), None, None, ok["default_next"].ctypes.data_as(C.c_void_p))
    assert eng.lib.vc_request_constraint(eng._model, C.byref(req)) == -1
    assert torch.equal(_gen(model, ids, px), plain), "a refused request changed the next call"


def check_true_dims(n_items=133, n_new=24):
    """7b dims (V = 32000), 2 decoder + 3 ViT layers, synthetic weights, B = 1: a from_list automaton over 133 id sequences — the
    device loop returns what a host loop over prefill + decode_step returns under the automaton's callable"""
    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine

    cfg = vcfg.vicuna_7b("vcoder_ds")
    cfg.num_hidden_layers = 2
    cfg.vit_num_layers = 3
    V = cfg.vocab_size
    rng = np.random.RandomState(5)
    pool = [int(t) for t in rng.choice(np.arange(1000, V), size=3 * n_items + 8, replace=False)]
    items = [pool[3 * i: 3 * i + 1 + i % 3] for i in range(n_items)]
    firsts = pool[3 * n_items:]
    a = TokenAutomaton.from_list([firsts[0]], items, [firsts[1]], [firsts[2]], [firsts[3]], min_items=3)
    eng = HipEngine(cfg)
    try:
        eng.load_synthetic(21)
        eng.finalize()
        ids = np.stack([synth.synth_prompt_ids(V, "vcoder_ds", sample=0)])
        px = synth.synth_batch(1, 336)
        T = ids.shape[1]
        plain = eng.generate(ids, *px, max_new_tokens=n_new)
        assert a.walk(plain[0].tolist()) == -1, "precondition: the unconstrained row is accepted"
        dev = eng.generate(ids, *px, max_new_tokens=n_new, constraint=a)
        assert int(eng.lib.vc_last_spliced_len(eng._model)) == 1216
        fn = a.as_prefix_allowed_tokens_fn(T, V)
        last, _, _ = eng.prefill(ids, *px, has_attention_mask=True, reserve=n_new)
        eng.clear_attention_mask()
        cur, host = torch.from_numpy(ids), []
        logits = torch.from_numpy(last).float()
        for step in range(n_new):
            nxt = torch.argmax(lp.apply_prefix_constraint(fn, cur, logits), dim=-1)
            host.append(int(nxt[0]))
            cur = torch.cat([cur, nxt[:, None]], dim=1)
            if step + 1 < n_new:
                logits = torch.from_numpy(eng.decode_step(nxt.numpy().astype(np.int32))[0]).float()
        print(f"7b dims, {a.num_states} states / {a.num_edges} edges: device {dev[0].tolist()}")
        assert dev[0].tolist() == host, f"7b dims: device {dev[0].tolist()}, host loop {host}"
        assert a.walk(host) >= 0
        assert np.array_equal(eng.generate(ids, *px, max_new_tokens=n_new), plain), "a plain call behind the constrained one differs"
    finally:
        eng.close()
