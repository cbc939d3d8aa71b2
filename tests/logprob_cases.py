"""Per-token log-probs and top-K alternatives (vck_topk_logprob, vc_request_generate_logprobs / vc_request_top_logprobs,
generate(output_logprobs=, top_logprobs=), score(top_logprobs=)): the checks shared by the CPU-emulator tests
(tests/test_logprobs_emu.py) and the `-m gpu` tests (tests/test_gpu_logprobs.py).  Every reference is numpy float64 over the same fp32
logits: log-softmax, and np.lexsort((ids, -values)) for the order (value descending, id ascending)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import e2e_cases
import kernel_cases as kc
import score_cases as sc
from score_cases import KERNEL_BAR, IGNORE

# ---- kernel ------------------------------------------------------------------------------------------------------------------
# Largest deviation of vck_topk_logprob (chosen_lp and top_lp; the staged and the unstaged path are bit-equal) from float64 over the
# shapes below: 2.38e-6 on the CPU emulator (libm expf / logf; the MI355X figure is in profiles/logprobs_wall_times.md).  The bar is
# score_cases.KERNEL_BAR (4.8e-6): the arithmetic is vck_token_logprob's (lse_add / lse_merge, expf / logf) with 1024 partial pairs per row.
KERNEL_SHAPES_EMU = [(1, 320, 320, 0), (5, 321, 352, 0), (33, 1000, 1003, 0), (2, 20, 24, 0)]   # (rows, V, ldl, shift); the last: V < K
KERNEL_SHAPES_GPU = KERNEL_SHAPES_EMU + [(3, 32000, 32000, 0), (9, 32003, 32064, 1)]
KS = [0, 1, 5, 32]
KINDS = sc.KINDS + ["ties", "all_equal", "few_finite", "chosen_ninf", "chosen_negative"]
MAX_TOP = 32


def _row(kind, V, rng):
    """-> (fp32 row, chosen id)"""
    if kind in sc.KINDS:
        v, t, _ = sc._row(kind, V, rng)
        return v, t
    v = (rng.randn(V) * 3).astype(np.float32)
    t = int(rng.randint(0, V))
    if kind == "ties":   # 8 levels (0.0 and -0.0 among them): the K-th boundary falls inside a tie group for every K < V
        v = (np.round(np.clip(rng.randn(V), -1.9, 1.9) * 2) / 2).astype(np.float32)
    elif kind == "all_equal":
        v[:] = np.float32(-2.25)
    elif kind == "few_finite":
        keep = rng.permutation(V)[:3]
        w = np.full(V, -np.inf, dtype=np.float32)
        w[keep] = v[keep]
        v, t = w, int(keep[1])
    elif kind == "chosen_ninf":
        v[t] = -np.inf
    elif kind == "chosen_negative":
        t = -1
    return v, t


def ref_topk(v, K):
    """float64 reference of one fp32 row -> (ids [K] with -1 behind the finite entries, log-probs [K] with -inf there, lse)"""
    v64 = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lse = np.logaddexp.reduce(v64)
    order = np.lexsort((np.arange(v64.size), -v64))[:K]
    order = order[np.isfinite(v64[order])]
    ids = np.full(K, -1, dtype=np.int64)
    lp = np.full(K, -np.inf, dtype=np.float64)
    ids[: order.size] = order
    lp[: order.size] = v64[order] - lse
    return ids, lp, lse


def compare_topk(what, v, K, got_ids, got_lp, bar=KERNEL_BAR):
    """one row's K entries against ref_topk: ids exact, values within the bar, non-increasing.  -> largest deviation"""
    ids, lp, _ = ref_topk(v, K)
    assert np.array_equal(np.asarray(got_ids, dtype=np.int64), ids), f"{what}: top ids {list(got_ids)}, expected {list(ids)}"
    got = np.asarray(got_lp, dtype=np.float64)
    fin = ids >= 0
    assert (got[~fin] == -np.inf).all(), f"{what}: slots behind the finite entries hold {got[~fin]}"
    assert np.isfinite(got[fin]).all(), f"{what}: {got[fin]}"
    assert (got[1:] <= got[:-1]).all(), f"{what}: top log-probs increase: {got}"
    dev = float(np.abs(got[fin] - lp[fin]).max()) if fin.any() else 0.0
    assert dev < bar, f"{what}: top log-probs deviate from float64 by {dev} (bar {bar})"
    return dev


def check_topk_logprob(be, rows, V, ldl, shift, K, seed=0):
    """every kind of row through launches of `rows` rows each, staged and unstaged; pad columns, the floats in front of the first row
    and behind the last hold NaN.  -> largest |deviation| from float64 over the finite values"""
    rng = np.random.RandomState(seed + rows * 7 + V + K)
    worst = 0.0
    n_launch = max(1, -(-len(KINDS) // rows))
    Kb = max(K, 1)
    for launch in range(n_launch):
        kinds = [KINDS[(launch * rows + r) % len(KINDS)] for r in range(rows)]
        buf = np.full(shift + rows * ldl + 3, np.nan, dtype=np.float32)
        chosen = np.zeros(rows, dtype=np.int32)
        vs = []
        for r, kind in enumerate(kinds):
            v, chosen[r] = _row(kind, V, rng)
            buf[shift + r * ldl: shift + r * ldl + V] = v
            vs.append(v)
        d_buf, d_ch = be.f32(buf), be.i32(chosen)
        res = []
        for lds in (-1, 0):
            # one row more than the launch writes: it must stay as it is
            d_clp = be.f32(np.full(rows + 1, np.nan, dtype=np.float32))
            d_tlp = be.f32(np.full((rows + 1) * Kb, np.nan, dtype=np.float32))
            d_tid = be.i32(np.full((rows + 1) * Kb, -7, dtype=np.int32))
            kc._call(be, "vck_topk_logprob", d_buf[shift:], ldl, d_ch, d_clp, d_tlp, d_tid, rows, V, K, lds)
            res.append((be.host_f32(d_clp).copy(), be.host_f32(d_tlp).copy(), be.host_i32(d_tid).copy()))
        for a, b in zip(res[0], res[1]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the staged and the unstaged path differ in bits"
        clp, tlp, tid = res[0]
        assert np.isnan(clp[rows]) and np.isnan(tlp[rows * Kb:]).all() and (tid[rows * Kb:] == -7).all(), "wrote past its rows"
        if K == 0:
            assert np.isnan(tlp).all() and (tid == -7).all(), "K = 0 wrote top entries"
        for r, kind in enumerate(kinds):
            what = f"topk_logprob rows {rows} V {V} ldl {ldl} shift {shift} K {K} row {r} ({kind})"
            v, t = vs[r], int(chosen[r])
            ids, lp, lse = ref_topk(v, K)
            ids_g, lp_g = tid[r * Kb: r * Kb + K], tlp[r * Kb: r * Kb + K]
            worst = max(worst, compare_topk(what, v, K, ids_g, lp_g))
            if kind == "all_equal":
                assert list(ids_g) == list(range(min(K, V))) + [-1] * max(K - V, 0), f"{what}: {ids_g}"
                assert np.abs(lp_g[: min(K, V)].astype(np.float64) + np.log(float(V))).max(initial=0.0) < KERNEL_BAR
            if kind == "few_finite":
                assert int((ids_g >= 0).sum()) == min(K, 3), f"{what}: {ids_g}"
            if t < 0:
                assert clp[r] == 0.0, f"{what}: chosen < 0 gives {clp[r]}"
            elif v[t] == -np.inf:
                assert clp[r] == -np.inf, f"{what}: a -inf logit gives {clp[r]}"
            else:
                dev = abs(float(clp[r]) - (float(v[t]) - lse))
                worst = max(worst, dev)
                assert dev < KERNEL_BAR, f"{what}: chosen log-prob deviates from float64 by {dev}"
                hit = np.nonzero(ids_g == t)[0]
                if hit.size:
                    assert clp[r: r + 1].view(np.int32)[0] == lp_g[hit[0]: hit[0] + 1].view(np.int32)[0], \
                        f"{what}: chosen_lp {clp[r]!r} and the top entry of the same id {lp_g[hit[0]]!r} differ in bits"
    # chosen == NULL: every row 0.0, the top entries as before
    d_clp = be.f32(np.full(rows, np.nan, dtype=np.float32))
    d_tlp = be.f32(np.full(rows * Kb, np.nan, dtype=np.float32))
    d_tid = be.i32(np.full(rows * Kb, -7, dtype=np.int32))
    kc._call(be, "vck_topk_logprob", d_buf[shift:], ldl, None, d_clp, d_tlp, d_tid, rows, V, K, -1)
    assert (be.host_f32(d_clp) == 0.0).all()
    if K:
        assert np.array_equal(be.host_i32(d_tid), tid[: rows * Kb])
    print(f"topk_logprob rows {rows} V {V} ldl {ldl} shift {shift} K {K}: largest deviation from float64 {worst:.3e} (bar {KERNEL_BAR:.1e})")
    return worst


# ---- engine and model ------------------------------------------------------------------------------------------------------------
N_NEW = 6
TOP = 5
model_for = sc.model_for


def inputs_for(B, V=None):
    """B = 2: a multimodal fixture prompt; B = 3: text-only random ids.  -> (ids [B, T] int64, kwargs of images / segs / depths)"""
    t = lambda a: None if a is None else torch.from_numpy(a)
    if B == 2:
        g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs("ds_img_depth_seg")
        return ids, dict(images=t(imgs), segs=t(segs), depths=t(deps))
    ids = np.random.RandomState(B).randint(3, V, size=(B, 12)).astype(np.int64)
    return ids, dict(images=None)


def replay_logits(model, ids, px, new):
    """the engine's own logits of every step of a generate() call: prefill, then decode_step over the generated ids.  -> [n, B, V]"""
    eng = model.engine
    last, _, _ = eng.prefill(ids, px.get("images"), px.get("segs"), px.get("depths"), has_attention_mask=True, reserve=new.shape[1])
    eng.clear_attention_mask()
    model._generation += 1
    steps = [last.copy()]
    for s_ in range(new.shape[1] - 1):
        lg, _ = eng.decode_step(new[:, s_].astype(np.int32))
        steps.append(lg.copy())
    return np.stack(steps, 0)


def finish_cols(new, eos=None, stops=()):
    """columns of every row up to and including its finishing token (n when it never finishes; prompt tails play no part here)"""
    B, n = new.shape
    end = np.full(B, n)
    for b in range(B):
        for s_ in range(n):
            hit = eos is not None and new[b, s_] == eos
            for q in stops:
                hit = hit or (s_ + 1 >= len(q) and list(new[b, s_ + 1 - len(q): s_ + 1]) == list(q))
            if hit:
                end[b] = s_ + 1
                break
    return end


def check_fields(what, new, tok_lp, top_lp, top_id, end, greedy, logits=None, K=TOP):
    """the fields of one call: scored up to the finishing token (greedy: top id 0 = the token, bit-equal log-probs), 0.0 / 0.0 / -1
    behind it; with `logits` [n, B, V]: ids exact and values within KERNEL_BAR of float64 over them.  -> largest deviation"""
    B, n = new.shape
    assert tok_lp.shape == (B, n) and tok_lp.dtype == np.float32
    assert top_lp.shape == (B, n, K) and top_id.shape == (B, n, K)
    worst = 0.0
    for b in range(B):
        for s_ in range(n):
            w = f"{what} row {b} step {s_}"
            if s_ >= end[b]:
                assert tok_lp[b, s_] == 0.0 and (top_lp[b, s_] == 0.0).all() and (top_id[b, s_] == -1).all(), \
                    f"{w}: behind the finishing token: {tok_lp[b, s_]} {top_lp[b, s_]} {top_id[b, s_]}"
                continue
            assert tok_lp[b, s_] < 0.0 or (tok_lp[b, s_] == 0.0 and logits is not None), f"{w}: log-prob {tok_lp[b, s_]}"
            if greedy and K:
                assert top_id[b, s_, 0] == new[b, s_], f"{w}: greedy token {new[b, s_]}, most likely {top_id[b, s_, 0]}"
                assert tok_lp[b, s_: s_ + 1].view(np.int32)[0] == top_lp[b, s_, :1].view(np.int32)[0], f"{w}: not bit-equal"
            if logits is not None:
                v = logits[s_, b]
                if K:
                    worst = max(worst, compare_topk(w, v, K, top_id[b, s_], top_lp[b, s_]))
                _, _, lse = ref_topk(v, 0)
                dev = abs(float(tok_lp[b, s_]) - (float(v[new[b, s_]]) - lse))
                worst = max(worst, dev)
                assert dev < KERNEL_BAR, f"{w}: token log-prob deviates from float64 over the engine's logits by {dev}"
                hit = np.nonzero(top_id[b, s_] == new[b, s_])[0]
                if hit.size:
                    assert tok_lp[b, s_: s_ + 1].view(np.int32)[0] == top_lp[b, s_, hit[0]: hit[0] + 1].view(np.int32)[0], f"{w}: not bit-equal"
    return worst


def _np(out):
    return (out.token_logprobs.numpy(), out.top_logprobs.numpy(), out.top_token_ids.numpy())


def check_generate(model, mode, B, sample=False):
    """a, b, c: ids with and without the request; greedy consistency; every field against the engine's own replayed logits"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B, model.config.vocab_size)
        T = ids.shape[1]
        kw = dict(max_new_tokens=N_NEW, eos_token_id=-1, do_sample=sample, **px)
        if sample:
            kw.update(temperature=0.8, top_k=20, top_p=0.9, seed=7)
        t_ids = torch.from_numpy(ids)
        plain = model.generate(t_ids, **kw)
        assert isinstance(plain, torch.Tensor)
        out = model.generate(t_ids, output_logprobs=True, top_logprobs=TOP, **kw)
        assert torch.equal(out.sequences, plain) and torch.equal(out[0], plain) and out["sequences"] is out.sequences, \
            "the ids change with the log-prob request"
        new = out.sequences[:, T:].numpy()
        tok_lp, top_lp, top_id = _np(out)
        assert out.top_token_ids.dtype == torch.int64 and out.token_logprobs.dtype == torch.float32
        assert torch.equal(out.sequence_logprob, out.token_logprobs.sum(1))
        lg = replay_logits(model, ids, px, new)
        worst = check_fields(f"generate [{mode}] B {B} sample {sample}", new, tok_lp, top_lp, top_id, np.full(B, N_NEW), not sample, lg)
        print(f"generate [{mode}] B {B} sample {sample}: largest deviation from float64 over the engine's own logits {worst:.3e}")
        only = model.generate(t_ids, output_logprobs=True, **kw)   # K = 0: no top fields, the same token log-probs
        assert only.top_logprobs is None and only.top_token_ids is None
        assert np.array_equal(only.token_logprobs.numpy().view(np.int32), tok_lp.view(np.int32))
        bare = model.generate(t_ids, return_dict_in_generate=True, **kw)
        assert torch.equal(bare.sequences, plain) and bare.token_logprobs is None and bare.sequence_logprob is None
        return worst
    finally:
        eng.set_precision("bf16")


def check_finishing(model, B=2):
    """d: an EOS and a 2-token stop sequence met at step 2 of row 0: scored there, 0.0 / -1 behind, the other rows go on"""
    eng = model.engine
    ids, px = inputs_for(B, model.config.vocab_size)
    args = (ids, px.get("images"), px.get("segs"), px.get("depths"))
    base = eng.generate(*args, max_new_tokens=N_NEW)
    eos = int(base[0, 2])
    for kw, fin in ((dict(eos_token_id=eos, pad_token_id=0), dict(eos=eos)),
                    (dict(stop_sequences=[[int(base[0, 1]), int(base[0, 2])]], pad_token_id=0), dict(stops=[[int(base[0, 1]), int(base[0, 2])]]))):
        plain = eng.generate(*args, max_new_tokens=N_NEW, **kw)
        new = eng.generate(*args, max_new_tokens=N_NEW, logprobs=True, top_logprobs=TOP, **kw)
        assert np.array_equal(new, plain)
        end = finish_cols(new, **fin)
        assert end[0] <= 3 and end.max() == new.shape[1]
        assert (end > 3).any(), "every row finishes with row 0: nothing shows that the other rows go on"
        lg = replay_logits(model, ids, px, np.where(np.arange(new.shape[1])[None] < end[:, None], new, base[:, : new.shape[1]]))
        check_fields(f"finishing {list(kw)[0]}", new, *eng.last_generate_logprobs, end, True, None)
        # scored positions against the replay (rows behind their finishing token are fed pad in the loop: not compared)
        tok_lp, top_lp, top_id = eng.last_generate_logprobs
        for b in range(B):
            for s_ in range(int(end[b])):
                compare_topk(f"finishing row {b} step {s_}", lg[s_, b], TOP, top_id[b, s_], top_lp[b, s_])
        out = model.generate(torch.from_numpy(ids), max_new_tokens=N_NEW, top_logprobs=TOP, **px,
                             **({"eos_token_id": eos, "pad_token_id": 0} if "eos_token_id" in kw else
                                {"eos_token_id": -1, "pad_token_id": 0, "stopping_criteria": [_DeviceStop(kw["stop_sequences"])]}))
        assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), new)
        assert np.array_equal(out.token_logprobs.numpy().view(np.int32), tok_lp.view(np.int32))
        assert np.array_equal(out.top_token_ids.numpy(), top_id)


class _DeviceStop:
    def __init__(self, seqs):
        self.seqs = seqs

    def device_stop_sequences(self):
        return self.seqs


def check_streaming(model, B=2):
    """e: on_tokens sees the same ids with the request as without it, and the ids returned"""
    eng = model.engine
    ids, px = inputs_for(B, model.config.vocab_size)
    args = (ids, px.get("images"), px.get("segs"), px.get("depths"))
    seen = {}
    for lp in (False, True):
        got = []
        new = eng.generate(*args, max_new_tokens=N_NEW, on_tokens=lambda first, a: got.append((first, a.copy())), stream_every=2,
                           logprobs=lp, top_logprobs=TOP if lp else 0)
        seen[lp] = (new, got)
        assert np.array_equal(np.concatenate([a for _, a in got], 1), new)
    assert np.array_equal(seen[False][0], seen[True][0])
    for new, got in seen.values():   # (how the columns are cut into reports is the loop's business: the pool and a session differ)
        assert [f for f, _ in got] == list(np.cumsum([0] + [a.shape[1] for _, a in got[:-1]]))

    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got.append(v.clone())

        def end(self):
            pass

    s0, s1 = Streamer(), Streamer()
    t_ids = torch.from_numpy(ids)
    model.generate(t_ids, max_new_tokens=N_NEW, eos_token_id=-1, streamer=s0, **px)
    model.generate(t_ids, max_new_tokens=N_NEW, eos_token_id=-1, streamer=s1, top_logprobs=2, **px)
    assert len(s0.got) == len(s1.got) == N_NEW + 1 and all(torch.equal(a, b) for a, b in zip(s0.got, s1.got))


def check_followed_by_plain(model, mode="bf16", B=2):
    """f: a plain decode_step and a plain generate behind a log-prob generate give what they give without it"""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B, model.config.vocab_size)
        args = (ids, px.get("images"), px.get("segs"), px.get("depths"))
        plain = eng.generate(*args, max_new_tokens=N_NEW)
        want = replay_logits(model, ids, px, plain[:, :5])[-1]     # logits behind tokens 0 .. 3: the step that takes token 3
        want2, _ = eng.decode_step(plain[:, 4].astype(np.int32))
        new = eng.generate(*args, max_new_tokens=4, logprobs=True, top_logprobs=TOP)
        assert np.array_equal(new, plain[:, :4])
        eng._step_pos = 0
        got, nxt = eng.decode_step(plain[:, 3].astype(np.int32))   # the session's loop stands behind token 2
        assert np.array_equal(got, want), "a plain decode_step behind a log-prob generate differs"
        got2, _ = eng.decode_step(None)                             # ... and continues from the token selected on the device
        assert np.array_equal(nxt, plain[:, 4]) and np.array_equal(got2, want2)
        again = eng.generate(*args, max_new_tokens=N_NEW)
        assert np.array_equal(again, plain) and eng.last_generate_logprobs is None
        # a larger max_new than any call before (the slabs grow) and another K (another captured step)
        more = eng.generate(*args, max_new_tokens=N_NEW + 3, logprobs=True, top_logprobs=2)
        assert np.array_equal(more[:, :N_NEW], plain) and eng.last_generate_logprobs[1].shape == (B, N_NEW + 3, 2)
        # decode_step(None) directly behind a call with log-probs AND a processor: the plain step (raw logits, greedy choice), from the
        # token that call selected on the device
        from vcoder_amd import logits_processors
        proc = logits_processors.make(repetition_penalty=1.3, bad_words_ids=[[int(plain[0, 1])]])
        new = eng.generate(*args, max_new_tokens=4, logprobs=True, top_logprobs=2, processors=proc)
        assert new.shape == (B, 4) and new[0, 1] != plain[0, 1], "the processors change nothing: the case shows nothing"
        got3, nxt3 = eng.decode_step(None)
        want3 = replay_logits(model, ids, px, np.concatenate([new, new[:, :1]], axis=1))[-1]   # the logits behind tokens 0 .. 3
        assert np.array_equal(got3, want3), "a plain decode_step behind a log-prob + processor generate differs"
        assert np.array_equal(nxt3, np.argmax(want3, axis=1)), "the plain step behind a processed call ran the processors"
    finally:
        eng.set_precision("bf16")


def own_top(logits, labels, K):
    """float64 reference of score(top_logprobs=K) over all-row logits [B, S, V]: -> {(b, j): (ids, lp)} of the scored positions"""
    out = {}
    for b, j in zip(*np.nonzero(labels[:, 1:] != IGNORE)):
        out[(int(b), int(j) + 1)] = ref_topk(logits[b, j], K)[:2]
    return out


def compare_score_top(what, sc_out, logits, labels, K, bar=KERNEL_BAR):
    tlp, tid = sc_out.top_logprobs.numpy(), sc_out.top_token_ids.numpy()
    assert tlp.shape == labels.shape + (K,) and tid.shape == tlp.shape and sc_out.top_token_ids.dtype == torch.int64
    scored = np.zeros(labels.shape, dtype=bool)
    worst = 0.0
    for (b, j) in own_top(logits, labels, K):
        scored[b, j] = True
        worst = max(worst, compare_topk(f"{what} position ({b}, {j})", logits[b, j - 1], K, tid[b, j], tlp[b, j], bar))
        hit = np.nonzero(tid[b, j] == labels[b, j])[0]
        if hit.size:   # the label among the alternatives: the same bits as its token log-prob
            assert sc_out.token_logprobs.numpy()[b, j: j + 1].view(np.int32)[0] == tlp[b, j, hit[0]: hit[0] + 1].view(np.int32)[0]
    assert (tlp[~scored] == 0.0).all() and (tid[~scored] == -1).all(), f"{what}: an unscored position carries alternatives"
    print(f"{what}: {int(scored.sum())} scored positions, largest deviation {worst:.3e} (bar {bar:.1e})")
    return worst


def check_score_text_only(model, B, T, per_row, K=3):
    V = model.config.vocab_size
    rng = np.random.RandomState(T + B + per_row)
    ids = rng.randint(3, V, size=(B, T)).astype(np.int64)
    labels = np.full((B, T), IGNORE, dtype=np.int64)
    for b in range(B):
        pos = rng.choice(np.arange(1, T), size=per_row, replace=False)
        labels[b, pos] = ids[b, pos]
    t = torch.from_numpy
    out = model(input_ids=t(ids), labels=t(labels))
    s = model.score(t(ids), t(labels), top_logprobs=K)
    plain = model.score(t(ids), t(labels))
    assert plain.top_logprobs is None and plain.top_token_ids is None
    assert np.array_equal(plain.token_logprobs.numpy().view(np.int32), s.token_logprobs.numpy().view(np.int32))
    return compare_score_top(f"score text-only B {B} T {T} per row {per_row}", s, out.logits.numpy(), labels, K)


def check_score_case(model, name="ds_img_seg_depth", K=3):
    variant, ids, labels, imgs, segs, deps = sc.case_inputs(name)
    t = torch.from_numpy
    out = model(input_ids=t(ids), labels=t(labels), images=imgs, segs=segs, depths=deps)
    s = model.score(t(ids), t(labels), images=imgs, segs=segs, depths=deps, top_logprobs=K)
    return compare_score_top(f"score {name}", s, out.logits.numpy(), s.labels.numpy(), K)


def check_score_continuation(model, mode="bf16", n=9, K=3):
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(2)
        t = torch.from_numpy
        pre = model(input_ids=t(ids), use_cache=True, **px)
        pkv = pre.past_key_values
        S = pkv.length
        cand = np.random.RandomState(n).randint(3, model.config.vocab_size, size=(2, n)).astype(np.int64)
        labels = cand.copy()
        labels[0, 3] = IGNORE
        out = model(input_ids=t(cand), past_key_values=pkv)
        pkv.crop(S)
        s = model.score(t(cand), t(labels), past_key_values=pkv, top_logprobs=K)
        return compare_score_top(f"score continuation [{mode}]", s, out.logits.numpy(), labels, K)
    finally:
        eng.set_precision("bf16")


def check_host_fallback(model, B=2):
    """h: a stopping criterion that needs host code: the per-token loop gives the same fields — against its own logits (which are the
    replay's), with EOS masking; and, over logits quantised to ties, the order (value descending, id ascending)"""
    eng = model.engine
    ids, px = inputs_for(B, model.config.vocab_size)
    T = ids.shape[1]
    t_ids = torch.from_numpy(ids)

    class Never:
        def __call__(self, output_ids, scores, **kw):
            return False

    base = model.generate(t_ids, max_new_tokens=N_NEW, eos_token_id=-1, **px)[:, T:].numpy()
    eos = int(base[0, 2])
    dev = model.generate(t_ids, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=0, top_logprobs=TOP, **px)
    out = model.generate(t_ids, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=0, top_logprobs=TOP, stopping_criteria=[Never()], **px)
    assert torch.equal(out.sequences, dev.sequences)
    new = out.sequences[:, T:].numpy()
    end = finish_cols(new, eos=eos)
    lg = replay_logits(model, ids, px, np.where(np.arange(new.shape[1])[None] < end[:, None], new, base[:, : new.shape[1]]))
    for b in range(B):   # rows behind their finishing token are fed pad: their logits are not the replay's, and nothing is scored there
        lg[int(end[b]):, b] = 0.0
    check_fields("host fallback", new, *_np(out), end, True, lg)
    assert np.array_equal(out.top_token_ids.numpy(), dev.top_token_ids.numpy())
    assert np.abs(out.token_logprobs.numpy() - dev.token_logprobs.numpy()).max() < 2 * KERNEL_BAR
    assert torch.equal(out.sequence_logprob, out.token_logprobs.sum(1))
    # ties: the loop sees logits rounded to halves
    real_prefill, real_step = eng.prefill, eng.decode_step
    seen = []

    def q(lg_):
        lg_ = (np.round(lg_ * 2) / 2).astype(np.float32)
        seen.append(lg_.copy())
        return lg_

    eng.prefill = lambda *a, **k: (lambda r: (q(r[0]),) + tuple(r[1:]))(real_prefill(*a, **k))
    eng.decode_step = lambda *a, **k: (lambda r: (q(r[0]),) + tuple(r[1:]))(real_step(*a, **k))
    try:
        tied = model.generate(t_ids, max_new_tokens=3, eos_token_id=-1, top_logprobs=TOP, stopping_criteria=[Never()], **px)
    finally:
        del eng.prefill, eng.decode_step
    check_fields("host fallback over tied logits", tied.sequences[:, T:].numpy(), *_np(tied), np.full(B, 3), True, np.stack(seen[:3], 0))


def check_refusals(model):
    """i: every refusal leaves the session's cache position and a live KVCacheHandle usable"""
    eng = model.engine
    ids, px = inputs_for(2)
    t = torch.from_numpy
    pre = model(input_ids=t(ids), use_cache=True, **px)
    pkv = pre.past_key_values
    tok = torch.from_numpy(np.random.RandomState(4).randint(3, model.config.vocab_size, size=(2, 1)))
    before = model(input_ids=tok, past_key_values=pkv, images=px["images"]).logits.numpy().copy()
    pkv.crop(pkv.length - 1)
    g = dict(max_new_tokens=3, eos_token_id=-1, **px)
    for kw, exc in ((dict(top_logprobs=33), ValueError), (dict(top_logprobs=-1), ValueError),
                    (dict(num_beams=2, output_logprobs=True), NotImplementedError), (dict(num_beams=2, top_logprobs=2), NotImplementedError),
                    (dict(output_scores=True, return_dict_in_generate=True), NotImplementedError)):
        try:
            model.generate(t(ids), **g, **kw)
            raise AssertionError(f"generate({kw}) was accepted")
        except exc as e:
            if "output_scores" in kw:
                assert "output_logprobs" in str(e)
    try:
        model.score(t(ids), t(ids), top_logprobs=33, **px)
        raise AssertionError("score(top_logprobs=33) was accepted")
    except ValueError:
        pass
    # at the C level: K outside 0 .. 32, a missing buffer, top-K without a pending score request; too small a cap_rows
    lp = np.full((2 * 3,), 7.0, dtype=np.float32)
    tl = np.full((2 * 3 * 2,), 7.0, dtype=np.float32)
    ti = np.full((2 * 3 * 2,), 7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert eng.lib.vc_request_generate_logprobs(eng._model, 33, p(lp), p(tl), p(ti), C.c_size_t(6)) == -1
    assert eng.lib.vc_request_generate_logprobs(eng._model, 2, p(lp), None, p(ti), C.c_size_t(6)) == -1
    assert eng.lib.vc_request_top_logprobs(eng._model, 2, p(tl), p(ti), C.c_size_t(tl.size)) == -3
    assert eng.lib.vc_request_generate_logprobs(eng._model, 2, p(lp), p(tl), p(ti), C.c_size_t(5)) == 0
    try:
        eng.generate(ids, px["images"], px["segs"], px["depths"], max_new_tokens=3)   # 2 x 3 rows into 5
        raise AssertionError("vc_generate accepted log-prob buffers that are too small")
    except ValueError:
        pass
    assert (lp == 7.0).all() and (tl == 7.0).all() and (ti == 7).all()
    after = model(input_ids=tok, past_key_values=pkv, images=px["images"]).logits.numpy()
    assert np.array_equal(before, after), "a refused call changed the cache of the live KVCacheHandle"
    # a request is one-shot: the failed call consumed it, a cancelled one never fires, another entry point clears it
    assert eng.lib.vc_request_generate_logprobs(eng._model, 2, p(lp), p(tl), p(ti), C.c_size_t(6)) == 0
    assert eng.lib.vc_request_generate_logprobs(eng._model, 0, None, None, None, C.c_size_t(0)) == 0
    eng.generate(ids, px["images"], px["segs"], px["depths"], max_new_tokens=3)
    assert eng.lib.vc_request_generate_logprobs(eng._model, 2, p(lp), p(tl), p(ti), C.c_size_t(6)) == 0
    eng.prefill(ids, px["images"], px["segs"], px["depths"])
    eng.generate(ids, px["images"], px["segs"], px["depths"], max_new_tokens=3)
    assert (lp == 7.0).all() and (tl == 7.0).all() and (ti == 7).all(), "a log-prob request outlived the call behind it"
    # accepted through the ABI alone: 2 x 3 rows
    assert eng.lib.vc_request_generate_logprobs(eng._model, 2, p(lp), p(tl), p(ti), C.c_size_t(6)) == 0
    new = eng.generate(ids, px["images"], px["segs"], px["depths"], max_new_tokens=3)
    assert (lp < 0).all() and np.array_equal(ti.reshape(2, 3, 2)[:, :, 0], new)
