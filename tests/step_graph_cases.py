"""The session's captured decode steps (csrc/engine.hip StepKey, engine_llm.inc step_graph): a step is replayed while the description it
was captured from is the one the call asks for, and re-captured — once, and only the kind of step the call uses — when anything it
bakes in has changed.  The checks shared by the CPU-emulator tests (tests/test_step_graph_emu.py) and the `-m gpu` tests
(tests/test_gpu_step_graph.py).

The four kinds of call that run on the session's own loop: a prefill + decode_step loop (the plain step), generate(logprobs=True) and
generate(<a processor>) (the call's own step), generate_beam (the beam step).  Captures are counted by vc_debug_step_captures
(HipEngine.step_captures).  Every result is compared bit for bit with what a fresh session (HipEngine.fork) returns that performs
only that call: a stale address or size in a replayed step shows there, whatever the counter says."""
from __future__ import annotations

import numpy as np

import logprob_cases as lc
from vcoder_amd import logits_processors as lp

N = 4          # steps of the base calls: 16 rows x 4 ids fill out_ids' first allocation exactly, so no base call grows it
model_for = lc.model_for


class Call:
    """one call on an engine -> a tuple of arrays; `name` identifies it (the fresh-session result is computed once per name)"""

    def __init__(self, name, fn, mode="bf16"):
        self.name, self.fn, self.mode = f"{mode}:{name}", fn, mode

    def __call__(self, eng):
        return self.fn(eng)


def _px(px):
    return px.get("images"), px.get("segs"), px.get("depths")


def text_inputs(B, T, V, seed=0):
    return np.random.RandomState(seed + 31 * B + T).randint(3, V, size=(B, T)).astype(np.int64), dict(images=None)


def loop(ids, px, steps=N, mask=None, reserve=N, mode="bf16", tag=""):
    """prefill, then `steps` decode_step(None): -> (logits of the prefill and of every step [steps + 1, B, V], chosen tokens)"""
    def fn(eng):
        last, _, _ = eng.prefill(ids, *_px(px), has_attention_mask=True, reserve=reserve, attention_mask=mask)
        lg, tok = [last], []
        for _ in range(steps):
            l, t = eng.decode_step(None)
            lg.append(l)
            tok.append(t)
        return np.stack(lg), np.stack(tok)
    return Call(f"loop{tag} B{ids.shape[0]} T{ids.shape[1]} steps{steps} reserve{reserve} mask{mask is not None}", fn, mode)


def gen(ids, px, max_new=N, K=None, proc=None, mode="bf16", tag=""):
    """generate on the session's loop with log-probs (K is not None) and / or processors: -> (ids, log-probs, top log-probs, top ids)"""
    def fn(eng):
        out = eng.generate(ids, *_px(px), max_new_tokens=max_new, logprobs=K is not None, top_logprobs=K or 0, processors=proc)
        return (out,) + tuple(eng.last_generate_logprobs or ())
    return Call(f"gen{tag} B{ids.shape[0]} T{ids.shape[1]} new{max_new} K{K} proc{proc is not None}", fn, mode)


def beam(ids, px, n=2, max_new=N, mode="bf16", tag=""):
    def fn(eng):
        return tuple(eng.generate_beam(ids, *_px(px), num_beams=n, max_new_tokens=max_new))
    return Call(f"beam{tag} B{ids.shape[0]} T{ids.shape[1]} n{n} new{max_new}", fn, mode)


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
                                    for x, y in zip(map(np.ascontiguousarray, a), map(np.ascontiguousarray, b)))


class Session:
    """a fresh session of the model's engine, the counter, and the fresh-session results of the calls made on it"""
    _ref = {}   # root engine (the key holds it alive: its id is never reused) -> {call name: result}

    def __init__(self, model):
        self.root = model.engine
        self.eng = self.root.fork()
        self.mode = "bf16"

    def close(self):
        self.eng.close()

    def _set_mode(self, eng, mode):
        if eng.precision != mode:
            eng.set_precision(mode)

    def ref(self, call):
        refs = Session._ref.setdefault(self.root, {})
        if call.name not in refs:
            f = self.root.fork()
            try:
                self._set_mode(f, call.mode)
                refs[call.name] = call(f)
            finally:
                f.close()
        return refs[call.name]

    def run(self, call, captures, why=""):
        """the call on this session: it performs exactly `captures` captures (an int, or a collection of allowed counts) and returns
        the fresh session's bits"""
        self._set_mode(self.eng, call.mode)
        c0 = self.eng.step_captures()
        out = call(self.eng)
        d = self.eng.step_captures() - c0
        print(f"{call.name}: {d} capture(s) {why}")
        allowed = (captures,) if isinstance(captures, int) else tuple(captures)
        assert d in allowed, f"{call.name} {why}: {d} captures, expected {allowed}"
        assert same(out, self.ref(call)), f"{call.name} {why}: differs from a fresh session's result"
        return d

    def changed(self, call, why, moved_only=False):
        """a call whose step bakes something in that the step of its kind was not captured with: one capture, then replays.
        moved_only: all that changed is that a buffer was allocated again — a capture if its address moved, which is the allocator's
        choice (none of its capacity is baked in: the same address is the same step)"""
        self.run(call, (0, 1) if moved_only else 1, f"({why})")
        self.run(call, 0, f"(again behind: {why})")


def base_calls(model, mode="bf16"):
    """the four kinds, sized alike — the same rows (the beam call: one sequence of two beams), the same S + N positions — so that none
    of them grows a buffer another one's step bakes in"""
    ids, px = lc.inputs_for(2)
    one = {k: (None if v is None else v[:1]) for k, v in px.items()}
    return [gen(ids, px, K=2, mode=mode), gen(ids, px, proc=lp.make(repetition_penalty=1.3), mode=mode),
            beam(ids[:1], one, n=2, mode=mode), loop(ids, px, mode=mode)]


def check_replay(model):
    """1: the same call twice — the second replays; the kinds round-robin after each has run — every call replays.  The session
    keeps ONE step per kind, and the log-prob call and the processor call are of one kind (the call's own step): round-robin with
    either of them adds nothing, and alternating between the two re-captures that one step — once per switch, never another kind's"""
    s = Session(model)
    try:
        with_lp, with_proc, beam_call, loop_call = base_calls(model)
        for c in (with_lp, with_proc, beam_call, loop_call):
            s.run(c, 1, "(the first of its kind)")
            s.run(c, 0, "(the same call again)")
        for own, switch in ((with_lp, 1), (with_proc, 1), (with_proc, 0)):
            for rnd in range(2):
                s.run(own, switch if rnd == 0 else 0, f"(round-robin {rnd}; the call's own step was last captured for the other request: {bool(switch)})")
                s.run(beam_call, 0, f"(round-robin {rnd})")
                s.run(loop_call, 0, f"(round-robin {rnd})")
    finally:
        s.close()


def check_recapture(model):
    """2: every change of something a step bakes in re-captures the step of the call's kind exactly once — and the call returns the
    fresh session's bits, before and after"""
    s = Session(model)
    V = model.config.vocab_size
    try:
        ids, px = lc.inputs_for(2)
        for c in base_calls(model):
            s.run(c, 1, "(the first of its kind)")
        # a larger max_new than any call before: out_ids and the slabs are allocated again
        s.changed(gen(ids, px, max_new=9, K=2), "max_new 4 -> 9: out_ids and the log-prob slabs grow", moved_only=True)
        s.changed(loop(ids, px, reserve=9), "out_ids was allocated again under the plain step", moved_only=True)
        # another K
        s.changed(gen(ids, px, max_new=9, K=5), "top_logprobs 2 -> 5")
        s.changed(gen(ids, px, max_new=9, K=2), "top_logprobs 5 -> 2: the same slabs, another lp_k")
        # processors on, then off, with log-probs on
        pen = lp.make(repetition_penalty=1.3)
        s.changed(gen(ids, px, max_new=9, K=2, proc=pen), "processors on, log-probs on")
        s.changed(gen(ids, px, max_new=9, K=2), "processors off, log-probs on")
        s.changed(gen(ids, px, max_new=9, proc=pen), "processors alone")
        # num_beams 2 -> 3 -> 2 (text-only prompts from here on: the rows of the cache change with them)
        tids, tpx = text_inputs(2, 12, V)
        s.changed(beam(tids, tpx, n=2), "the first beam call over these rows")
        s.changed(beam(tids, tpx, n=3), "num_beams 2 -> 3")
        s.changed(beam(tids, tpx, n=2), "num_beams 3 -> 2")
        # beam max_new across a multiple of 64: the tables and the permute staging hold cap_new = 128 steps
        s.changed(beam(tids, tpx, n=2, max_new=65), "beam max_new 4 -> 65")
        s.run(beam(tids, tpx, n=2), 0, "(a shorter beam call fits the larger tables)")
        # B 2 -> 3 -> 2: the 16-row-padded step buffers stay, the cache is allocated again
        t3, p3 = text_inputs(3, 12, V)
        s.changed(loop(tids, tpx), "the plain step over the text rows")
        s.changed(loop(t3, p3), "B 2 -> 3")
        s.changed(gen(t3, p3, K=2), "B 2 -> 3, the call's own step")
        s.changed(loop(tids, tpx), "B 3 -> 2")
        s.changed(gen(tids, tpx, K=2), "B 3 -> 2, the call's own step")
        # a masked prefill keeps its keys hidden in the decode_step loop; an unmasked one behind it does not
        mask = np.ones(tids.shape, dtype=np.uint8)
        mask[1, 3:5] = 0
        masked, unmasked = loop(tids, tpx, mask=mask), loop(tids, tpx)
        assert not same(s.ref(masked), s.ref(unmasked)), "the mask changes nothing: the case shows nothing"
        s.changed(masked, "a masked prefill")
        s.changed(unmasked, "an unmasked prefill")
        # precision mode "split" and back
        s.changed(loop(tids, tpx, mode="split"), "set_precision('split')")
        s.changed(gen(tids, tpx, K=2, mode="split"), "set_precision('split'), the call's own step")
        s.changed(loop(tids, tpx), "set_precision('bf16')")
    finally:
        s.eng.set_precision("bf16")
        s.close()


def check_grow_kv(model):
    """2, the decode_step loop that outruns its prefill's reserve: the cache is re-allocated under the loop (grow_kv), the step is
    captured once more, and the logits are those of a session whose prefill reserved enough"""
    V = model.config.vocab_size
    ids, px = text_inputs(2, 60, V)   # S = 60, reserve 2: a cache of 64 positions — the 5th step needs position 64
    root = model.engine
    a, b = root.fork(), root.fork()
    try:
        want = loop(ids, px, steps=7, reserve=32)(b)
        assert b.step_captures() == 1
        last, _, _ = a.prefill(ids, None, has_attention_mask=True, reserve=2)
        lg, tok = [last], []
        for step in range(7):
            c0 = a.step_captures()
            l, t = a.decode_step(None)
            lg.append(l)
            tok.append(t)
            d = a.step_captures() - c0
            assert d == (1 if step in (0, 4) else 0), f"step {step}: {d} captures (the first step and the one that grows the cache take one)"
        assert same((np.stack(lg), np.stack(tok)), want), "the loop across grow_kv differs from a loop whose prefill reserved enough"
    finally:
        a.close()
        b.close()


def check_plain_after_call(model, mode="bf16"):
    """3: decode_step(None) directly behind a generate with log-probs AND a processor continues from the token that call selected on
    the device, on the plain step — raw logits, greedy choice — and the same sequence again replays both steps"""
    s = Session(model)
    try:
        eng = s.eng
        eng.set_precision(mode)
        ids, px = lc.inputs_for(2)
        free = s.ref(gen(ids, px, mode=mode, tag="-free"))[0]
        proc = lp.make(repetition_penalty=1.3, bad_words_ids=[[int(free[0, 1])]])   # row 0 must leave the free-running ids at token 1
        call = gen(ids, px, K=2, proc=proc, mode=mode, tag="-badword")
        new = s.ref(call)[0]
        assert new.shape == (2, N) and not np.array_equal(new, free), "the processors change nothing: the case shows nothing"
        f = s.root.fork()
        try:
            f.set_precision(mode)
            f.prefill(ids, *_px(px), has_attention_mask=True, reserve=N + 1)
            for j in range(N):
                want, want_tok = f.decode_step(new[:, j].astype(np.int32))   # the last: logits behind tokens 0 .. N - 1
        finally:
            f.close()
        strict = mode == "strict"
        for rnd in range(2):
            s.run(call, 0 if strict or rnd else 1, f"(round {rnd})")
            c0 = eng.step_captures()
            got, tok = eng.decode_step(None)
            d = eng.step_captures() - c0
            assert d == (0 if strict or rnd else 1), f"round {rnd}: the plain step behind the call took {d} captures"
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), "the plain step behind the call: other logits"
            assert np.array_equal(tok, want_tok) and np.array_equal(tok, np.argmax(want, axis=1)), "the plain step ran the processors"
    finally:
        s.eng.set_precision("bf16")
        s.close()


def check_strict(model):
    """4: strict mode enqueues its steps eagerly — the calls return the fresh session's bits and nothing is ever captured"""
    s = Session(model)
    try:
        for c in base_calls(model, mode="strict")[:2] + [loop(*lc.inputs_for(2), mode="strict")]:
            s.run(c, 0, "(strict)")
            s.run(c, 0, "(strict, again)")
        assert s.eng.step_captures() == 0
    finally:
        s.eng.set_precision("bf16")
        s.close()
