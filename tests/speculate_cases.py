"""Prompt-lookup speculative decoding: cases shared by tests/test_speculate_emu.py (CPU emulator) and tests/test_gpu_speculate.py.

  vck_attention_verify  against Q launches of the per-row fused decode attention (vck_attention_decode_masked), one per query
                        position, on a copy of the same cache: output rows and cache bit-equal (an exactly-zero output may differ
                        in sign)
  vck_spec_draft        against draft_ref, the numpy statement of the drafting rule
  vck_spec_accept       against accept_ref, the numpy statement of the accepting rule and of the per-token bookkeeping
  generate(speculate=k) against the plain session loop: array_equal ids / n_generated / log-probs; the counters against simulate()
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

import kernel_cases as kc
from kernel_cases import RS, c_p, make_rows

MASK_STRIDE = 1024


# ---- attention_verify ------------------------------------------------------------------------------------------------------------
def stream_round(hd, kv8):
    """keys one round of the decode attention's 8 waves covers (attn.hip BATCH): rows in flight per lane x key rows per wave x 8"""
    epl = 16 if kv8 else 8
    uk = (6 if hd == 128 else 4) if kv8 else 8
    return 8 * (64 // (hd // epl)) * uk


def verify_positions(hd, kv8, Q, S):
    """the three chunk starts of the issue: 0, a chunk straddling one round of the key stream, a chunk ending at the capacity"""
    return {"zero": 0, "straddle": stream_round(hd, kv8) - max(Q // 2, 1), "end": S - Q}


def check_attention_verify(be, hd, B, Q, kv8, where=("straddle", "zero", "end"), nq=None, mask=False, seed=0, H=2):
    """row b of the launch: chunk start where[b % len(where)], nq[b] queries (default: Q, Q - 1 behind the first row).  The reference
    runs the plain kernel once per query position over its own copy of the cache, rows with j >= nq[b] inactive."""
    D = H * hd
    rng = np.random.RandomState(seed)
    S = stream_round(hd, kv8) + 72
    where = [where[b % len(where)] for b in range(B)]
    nq = list(nq) if nq is not None else [Q if b == 0 else max(Q - 1, 1) for b in range(B)]
    pos = []
    for b in range(B):
        p_ = verify_positions(hd, kv8, Q, S)[where[b]]
        pos.append(S - nq[b] if where[b] == "end" and nq[b] > 0 else p_)
    assert all(0 <= pos[b] and pos[b] + nq[b] <= S for b in range(B))
    scale = 1.0 / math.sqrt(hd)
    cos, sin = kc.rope_tables(S, hd)
    qkv = kc._op_decode(kc._op_bits(kc.bf16_round(rng.randn(B * Q, 3 * D)), be.operands), be.operands)
    k_old, v_old = rng.randn(B, H, S, hd).astype(np.float32), rng.randn(B, H, S, hd).astype(np.float32)
    enc = (lambda a: kc._u8_dev(be, kc.e4m3_bytes(a))) if kv8 else (lambda a: be.bf16(a))
    km = np.ones((B, MASK_STRIDE), np.uint8)
    if mask:
        for b in range(B):
            hide = rng.rand(pos[b]) < 0.3
            hide[:1] = False
            km[b, :pos[b]] = ~hide
    kmd = kc._u8_dev(be, km) if mask else None
    cd, sd = be.f32(cos), be.f32(sin)
    # ---- the verify launch
    kd, vd = enc(k_old), enc(v_old)
    k_init, v_init = kc.raw_bits(kd).copy(), kc.raw_bits(vd).copy()
    fill = 0x3F80   # an output row nothing writes keeps this pattern
    out = be.bits16(np.full((B * Q, D), fill, np.uint16))
    rec = np.zeros((B, 4), np.int32)
    rec[:, 1] = pos
    rd, nqd, qd = be.i32(rec), be.i32(nq), be.bf16(qkv)
    rc = be.lib.vck_attention_verify(be.ptr(qd), be.ptr(kd), be.ptr(vd), be.ptr(out), B, H, hd, S, Q, c_p(kc._addr(rd) + 4), 4, be.ptr(nqd),
                                     be.ptr(cd), be.ptr(sd), ctypes.c_float(scale), 3 if kv8 else 0, be.ptr(kmd), MASK_STRIDE, None)
    assert rc == 0
    be.sync()
    got, gk, gv = kc.raw_bits(out).reshape(B, Q, D), kc.raw_bits(kd), kc.raw_bits(vd)
    # ---- the reference: one plain step per query position
    kr, vr = enc(k_old), enc(v_old)
    ref = np.full((B, Q, D), fill, np.uint16)
    for j in range(max(nq)):
        rj = np.zeros((B, 4), np.int32)
        rj[:, 0] = [1 if j < nq[b] else 0 for b in range(B)]
        rj[:, 1] = [pos[b] + j for b in range(B)]
        rjd = be.i32(rj)
        qj = be.bf16(qkv.reshape(B, Q, 3 * D)[:, j])
        oj = be.bits16(np.full((B, D), fill, np.uint16))
        be.lib.vck_attention_decode_masked(be.ptr(qj), be.ptr(kr), be.ptr(vr), be.ptr(oj), B, H, hd, S, c_p(kc._addr(rjd) + 4), 4,
                                           c_p(kc._addr(rjd)), be.ptr(cd), be.ptr(sd), ctypes.c_float(scale), 3 if kv8 else 0, 0,
                                           be.ptr(kmd), MASK_STRIDE, None)
        be.sync()
        ref[:, j] = kc.raw_bits(oj).reshape(B, D)
    what = f"attention_verify hd{hd} B{B} Q{Q} kv8={kv8} where {where} nq {nq} mask={mask} [{be.operands}]"
    assert np.array_equal(gk, kc.raw_bits(kr)) and np.array_equal(gv, kc.raw_bits(vr)), f"{what}: cache rows differ"
    zero = (got & 0x7FFF) == 0
    same = (got == ref) | (zero & ((ref & 0x7FFF) == 0))
    assert same.all(), f"{what}: {np.count_nonzero(~same)} output elements differ, first at {np.argwhere(~same)[0]}"
    for b in range(B):
        assert (got[b, nq[b]:] == fill).all(), f"{what}: row {b} wrote behind its {nq[b]} queries"
        if nq[b] == 0:
            assert np.array_equal(gk.reshape(B, -1)[b], k_init.reshape(B, -1)[b]) and np.array_equal(gv.reshape(B, -1)[b], v_init.reshape(B, -1)[b])
    assert any((got[b, :nq[b]] != fill).any() for b in range(B) if nq[b]), f"{what}: nothing was written"


ATTN_VERIFY_CASES = [   # hd, B, Q, kv8, where, nq, mask
    (hd, B, Q, kv8, w, None, False)
    for hd in (128, 64) for kv8 in (0, 1) for B, w in ((1, ("straddle",)), (3, ("straddle", "zero", "end"))) for Q in (1, 2, 5, 8)
] + [
    (128, 1, 8, 0, ("zero",), None, False), (128, 1, 5, 1, ("end",), None, False), (64, 1, 8, 1, ("zero",), None, False),
    (64, 1, 2, 0, ("end",), None, False),
    (128, 3, 8, 0, ("end", "straddle", "zero"), (8, 0, 3), False),      # nq = 0: the row's cache and output stay untouched
    (128, 3, 5, 1, ("straddle", "end", "zero"), (2, 5, 0), True),
    (64, 3, 8, 0, ("straddle", "zero", "end"), (8, 6, 1), True),
    (128, 1, 8, 0, ("straddle",), None, True), (64, 3, 5, 1, ("end", "straddle", "straddle"), (5, 0, 4), True),
]


def check_attention_verify_volume(be, hd, kv8, seeds=(1, 2, 3)):
    """16 sequences x 8 heads x 8 queries per launch: a rounding of the fp32 arithmetic that differs from the decode kernel's shows
    in an output element only once in 2^13 (fp16 operands) to 2^16 (bf16) elements — the small shapes above cannot see it"""
    for seed in seeds:
        check_attention_verify(be, hd, 16, 8, kv8, nq=[8] * 16, seed=seed, H=8)


def check_attention_verify_refused(be):
    """the score rows of 8 queries over 4096 keys of an e4m3 hd-64 cache exceed a CU's LDS: nothing is launched"""
    assert be.lib.vck_attention_verify(None, None, None, None, 1, 1, 64, 4096, 9, None, 0, None, None, None, ctypes.c_float(1.0), 0, None, 0, None) == -1
    assert be.lib.vck_attention_verify(None, None, None, None, 1, 1, 64, 8192, 8, None, 0, None, None, None, ctypes.c_float(1.0), 1, None, 0, None) == -1


# ---- the rules, in numpy: the specification of spec_draft_kernel / spec_accept_kernel ---------------------------------------------
SEP = None   # the separator between the lookup ids and the prompt: no window may cover it, no draft may be it


def draft_ref(lookup, prompt, gen, k, max_ngram, V):
    """the drafts of one sequence: for ng = max_ngram .. 1 (an ng longer than prompt + generated is not tried) the last ng ids of
    lookup | SEP | prompt | generated are sought at every earlier start, the latest match of the first ng that has one decides, and
    the ids behind it are the drafts — at most k, cut at the corpus end and at the first id outside [0, V)"""
    corpus = [int(t) for t in lookup] + [SEP] + [int(t) for t in prompt] + [int(t) for t in gen]
    N = len(corpus)
    for ng in range(min(max_ngram, len(prompt) + len(gen)), 0, -1):
        tail, best = corpus[N - ng:], -1
        for s in range(N - ng):
            w = corpus[s:s + ng]
            if SEP not in w and w == tail:
                best = s
        if best >= 0:
            d = []
            for t in corpus[best + ng:]:
                if t is SEP or t < 0 or t >= V or len(d) >= k:
                    break
                d.append(t)
            return d
    return []


def emit_ref(r, sel):
    """the bookkeeping one selected token goes through (select.hip emit_token); r: dict(step, finished, eos, pad, stops, tail, out,
    max_new); tail = the 7 last prompt ids, right-aligned.  -> the token emitted"""
    can = r["eos"] >= 0 or len(r["stops"]) > 0
    was = r["finished"] if can else 0
    tok = sel
    if can:
        if was:
            tok = r["pad"]
        if r["eos"] >= 0 and tok == r["eos"]:
            r["finished"] = 1
    if r["step"] < r["max_new"]:
        r["out"][r["step"]] = tok
    if r["stops"] and not was:
        hist = list(r["tail"]) + list(r["out"][:r["step"]]) + [tok]
        if any(hist[-len(q):] == list(q) for q in r["stops"]):
            r["finished"] = 1
    return tok


def accept_ref(r, logits, tok, nq):
    """one sequence behind the lm_head of a verify step: a_j = argmax (lowest id on ties), the leading drafts tok[j] == a_(j-1) are
    accepted, a_0 .. a_n go through emit_ref one by one; a finishing token or the last slot cuts the rest.  r advances (step, pos).
    -> (last emitted id, [steps, emitted, drafted, emitted - 1])"""
    if nq <= 0:
        return None, [0, 0, 0, 0]
    a = [int(np.argmax(logits[j])) for j in range(nq)]
    emitted, last = 0, int(tok[0])
    for j in range(nq):
        if j > 0 and int(tok[j]) != a[j - 1]:
            break
        last = emit_ref(r, a[j])
        r["step"] += 1
        r["pos"] += 1
        emitted += 1
        if r["finished"] or r["step"] >= r["max_new"]:
            break
    return last, [1, emitted, nq - 1, emitted - 1]


def simulate(truth, lookup, prompt, k, max_ngram, V, eos=-1):
    """the counters [steps, tokens, drafted, accepted] of a speculated call whose plain output is `truth` (one row, max_new ids; no
    stop sequences): step 0 emits truth[0], every verify step drafts by draft_ref and accepts the leading drafts equal to truth"""
    max_new, n = len(truth), 1
    c = [0, 0, 0, 0]
    if eos >= 0 and truth[0] == eos:
        return c
    while n < max_new:
        d = draft_ref(lookup, prompt, truth[:n], k, max_ngram, V)[:min(k, max_new - n - 1)]
        emitted = 0
        for j in range(len(d) + 1):
            if j > 0 and d[j - 1] != truth[n + j - 1]:
                break
            emitted += 1
            if eos >= 0 and truth[n + j] == eos:
                break
        c = [c[0] + 1, c[1] + emitted, c[2] + len(d), c[3] + emitted - 1]
        n += emitted
        if eos >= 0 and truth[n - 1] == eos:
            break
    return c


# ---- spec_draft ------------------------------------------------------------------------------------------------------------------
V_SMALL = 64
PH = -200   # an image placeholder of the prompt

DRAFT_CASES = {   # name: (lookup, prompt, generated, k, max_ngram, max_new, finished)
    "no_match": ([40, 41], [1, 2, 3], [9], 3, 2, 16, 0),
    "match_only_at_ng1": ([], [5, 9, 7, 8], [6, 9], 3, 3, 16, 0),
    "latest_of_several": ([], [4, 5, 10, 4, 5, 11, 4, 5, 12, 13], [4, 5], 2, 2, 16, 0),
    "short_continuation": ([], [7, 8, 9], [3, 9], 5, 1, 16, 0),            # behind the match only "3, 9" is left
    # "2 | 3" across the separator is no match (its continuation would be 30, 31, 3): ng = 1 decides, the latest "3"
    "separator_not_straddled": ([1, 2], [3, 30, 31, 3, 40], [2, 3], 3, 2, 16, 0),
    "drafts_stop_at_separator": ([8, 9, 20], [1], [8, 9], 4, 2, 16, 0),
    "placeholders": ([], [1, PH, PH, 5, 6, PH, 7], [5], 4, 2, 16, 0),       # "5" matches; the drafts end in front of the placeholder
    "lookup_and_history": ([11, 12, 13, 14, 15, 16], [1, 2], [12, 13], 7, 2, 16, 0),
    "corpus_of_one_id": ([], [], [5], 3, 2, 16, 0),
    "finished_row": ([], [1, 2, 1, 2], [1, 2], 3, 2, 16, 1),
    "one_token_left": ([], [1, 2, 3, 1, 2, 3], [1, 2], 3, 2, 3, 0),
    "two_tokens_left": ([], [1, 2, 3, 4, 1, 2, 3, 4], [1, 2], 3, 2, 4, 0),
    "full_row": ([], [1, 2, 1, 2], [1, 2], 3, 2, 2, 0),
    "ngram_4": ([], [1, 2, 3, 4, 50, 9, 2, 3, 4, 51], [1, 2, 3, 4], 2, 4, 16, 0),
}


def check_spec_draft(be, names=None):
    """every case as one sequence of ONE launch (different corpora, lengths and records side by side)"""
    names = list(names or DRAFT_CASES)
    B, Q, pad = len(names), 8, 3
    cases = [DRAFT_CASES[n] for n in names]
    ls, ps, stride = max(len(c[0]) for c in cases) + 1, max(len(c[1]) for c in cases) + 1, 24
    rows = make_rows(B, PAD=pad, OUT_OFF=[b * stride for b in range(B)], MAXNEW=[c[5] for c in cases], STEP=[len(c[2]) for c in cases],
                     FINISHED=[c[6] for c in cases])
    out = np.full((B, stride), pad, np.int32)
    look, prm = np.full((B, ls), 17, np.int32), np.full((B, ps), 17, np.int32)   # behind a row's length: ids that must not be read
    for b, c in enumerate(cases):
        look[b, :len(c[0])], prm[b, :len(c[1])], out[b, :len(c[2])] = c[0], c[1], c[2]
    tok, nq = be.i32(np.full((B * Q,), -7)), be.i32(np.full((B,), -7))
    for k in sorted({c[3] for c in cases}):     # k and the n-gram size belong to a launch: one per distinct pair, the other rows ignored
        for ng in sorted({c[4] for c in cases if c[3] == k}):
            args = [be.i32(rows), be.i32(out), be.i32(look), be.i32([len(c[0]) for c in cases]), be.i32(prm), be.i32([len(c[1]) for c in cases])]
            be.lib.vck_spec_draft(be.ptr(args[0]), be.ptr(args[1]), be.ptr(args[2]), be.ptr(args[3]), ls, be.ptr(args[4]), be.ptr(args[5]), ps,
                                  be.ptr(tok), be.ptr(nq), B, Q, k, ng, V_SMALL, None)
            be.sync()
            g_tok, g_nq = be.host_i32(tok).reshape(B, Q), be.host_i32(nq)
            for b, (name, c) in enumerate(zip(names, cases)):
                if (c[3], c[4]) != (k, ng):
                    continue
                lookup, prompt, gen, _, _, max_new, fin = c
                if fin or len(gen) >= max_new:
                    want_nq, want = 0, [pad] * Q
                else:
                    d = draft_ref(lookup, prompt, gen, k, ng, V_SMALL)[:min(k, Q - 1, max_new - len(gen) - 1)]
                    want_nq, want = 1 + len(d), [gen[-1]] + d + [pad] * (Q - 1 - len(d))
                assert g_nq[b] == want_nq and list(g_tok[b]) == want, f"spec_draft {name}: nq {g_nq[b]} tok {list(g_tok[b])}, want {want_nq} {want}"
    # what the cases are there for
    ref = {n: draft_ref(*DRAFT_CASES[n][:3], DRAFT_CASES[n][3], DRAFT_CASES[n][4], V_SMALL) for n in DRAFT_CASES}
    assert ref["no_match"] == [] and ref["match_only_at_ng1"] == [7, 8, 6] and ref["latest_of_several"] == [12, 13]
    assert ref["short_continuation"] == [3, 9] and ref["separator_not_straddled"] == [40, 2, 3] and ref["drafts_stop_at_separator"] == [20]
    assert ref["placeholders"] == [6] and ref["corpus_of_one_id"] == [] and ref["lookup_and_history"] == [14, 15, 16]
    assert ref["ngram_4"] == [50, 9]


# ---- spec_accept -----------------------------------------------------------------------------------------------------------------
def _logits_for(rng, want, V, tie=None):
    """[len(want), V] rows whose argmax is want[j]; tie = (row, other id): that row's maximum is shared with `other`"""
    lg = rng.randn(len(want), V).astype(np.float32)
    for j, t in enumerate(want):
        lg[j, t] = lg[j].max() + 1.0
    if tie is not None:
        lg[tie[0], tie[1]] = lg[tie[0]].max()
    return lg


ACCEPT_CASES = {   # name: (tok row [last, drafts...], nq, argmax per row, record fields, tie)
    "all_accepted": ([5, 6, 7, 8], 4, [6, 7, 8, 9], {}, None),
    "none_accepted": ([5, 6, 7, 8], 4, [30, 7, 8, 9], {}, None),
    "some_accepted": ([5, 6, 7, 8], 4, [6, 7, 31, 9], {}, None),
    "no_drafts": ([5, 3, 3, 3], 1, [6, 7, 8, 9], {}, None),
    "eos_inside_run": ([5, 6, 7, 8], 4, [6, 7, 8, 9], dict(eos=7), None),
    "stop_completed_inside_run": ([5, 6, 7, 8], 4, [6, 7, 8, 9], dict(stops=[[40, 41, 6, 7]], tail=[0, 0, 0, 0, 0, 40, 41], step=0), None),
    "stop_with_history": ([5, 6, 7, 8], 4, [6, 7, 8, 9], dict(stops=[[12, 5, 6]], gen=[11, 12, 5]), None),
    "max_new_cut": ([5, 6, 7, 8], 4, [6, 7, 8, 9], dict(max_new=5, gen=[1, 2, 5]), None),
    "argmax_tie_lower_id_wins": ([5, 6, 7, 8], 4, [6, 7, 8, 9], {}, (0, 2)),       # row 0: ids 2 and 6 tie, 2 wins, draft 6 is rejected
    "argmax_tie_higher_id_loses": ([5, 6, 7, 8], 4, [6, 7, 8, 9], {}, (0, 50)),    # ids 6 and 50 tie, 6 wins, the run goes on
}


def check_spec_accept(be, logprobs=False):
    names = list(ACCEPT_CASES)
    B, Q, V, pad, stride, K = len(names), 4, V_SMALL, 3, 16, 3
    rng = np.random.RandomState(5)
    lg = np.zeros((B, Q, V), np.float32)
    rows = make_rows(B, PAD=pad, OUT_OFF=[b * stride for b in range(B)], MAXNEW=12)
    out = np.full((B, stride), pad, np.int32)
    toks, nqs, recs = np.zeros((B, Q), np.int32), np.zeros(B, np.int32), []
    for b, name in enumerate(names):
        tok, nq, want, f, tie = ACCEPT_CASES[name]
        lg[b] = _logits_for(rng, want, V, tie)
        toks[b], nqs[b] = tok, nq
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
    rd, od, nxt, cnt = be.i32(rows), be.i32(out), be.i32(np.full(B, -7)), be.i32(np.tile([10, 20, 30, 40], (B, 1)))
    lgd, td, nd = be.f32(lg.reshape(B * Q, V)), be.i32(toks), be.i32(nqs)
    s_lp = s_id = lp_tok = lp_top = lp_ids = None
    if logprobs:   # the scratch rows: any values will do — the kernel copies them
        s_lp_h, s_id_h = rng.randn(B * Q, K + 1).astype(np.float32), rng.randint(0, V, (B * Q, K + 1)).astype(np.int32)
        s_lp, s_id = be.f32(s_lp_h), be.i32(s_id_h)
        lp_tok, lp_top, lp_ids = be.f32(np.full((B * stride,), 7.0)), be.f32(np.full((B * stride, K), 7.0)), be.i32(np.full((B * stride, K), -7))
    be.lib.vck_spec_accept(be.ptr(lgd), V, V, be.ptr(rd), be.ptr(nxt), be.ptr(od), be.ptr(td), be.ptr(nd), B, Q, be.ptr(cnt), be.ptr(s_lp),
                           be.ptr(s_id), K + 1, be.ptr(lp_tok), be.ptr(lp_top), be.ptr(lp_ids), K if logprobs else 0, None)
    be.sync()
    g_rows, g_out, g_nxt, g_cnt = be.host_i32(rd), be.host_i32(od), be.host_i32(nxt), be.host_i32(cnt)
    emitted_of = {}
    for b, name in enumerate(names):
        r = recs[b]
        step0 = r["step"]
        last, c = accept_ref(r, lg[b], toks[b], int(nqs[b]))
        emitted_of[name] = c[1]
        w = f"spec_accept {name}"
        assert list(g_out[b]) == r["out"], f"{w}: ids {list(g_out[b])}, want {r['out']}"
        assert (g_rows[b, RS["STEP"]], g_rows[b, RS["POS"]], g_rows[b, RS["FINISHED"]]) == (r["step"], r["pos"], r["finished"]), \
            f"{w}: step / pos / finished {g_rows[b, 1:4]}, want {r['step']} {r['pos']} {r['finished']}"
        assert g_nxt[b] == last and list(g_cnt[b]) == [10 + c[0], 20 + c[1], 30 + c[2], 40 + c[3]], f"{w}: next {g_nxt[b]} counters {g_cnt[b]}"
        if logprobs:
            t, tp, ti = be.host_f32(lp_tok).reshape(B, stride), be.host_f32(lp_top).reshape(B, stride, K), be.host_i32(lp_ids).reshape(B, stride, K)
            for s_ in range(stride):
                j = s_ - step0
                if 0 <= j < c[1]:
                    assert t[b, s_] == s_lp_h[b * Q + j, 0] and np.array_equal(tp[b, s_], s_lp_h[b * Q + j, :K]) and \
                        np.array_equal(ti[b, s_], s_id_h[b * Q + j, :K]), f"{w}: log-prob slot {s_}"
                else:
                    assert t[b, s_] == 7.0 and (tp[b, s_] == 7.0).all() and (ti[b, s_] == -7).all(), f"{w}: slot {s_} was written"
    want = dict(all_accepted=4, none_accepted=1, some_accepted=3, no_drafts=1, eos_inside_run=2, stop_completed_inside_run=2,
                stop_with_history=1, max_new_cut=2, argmax_tie_lower_id_wins=1, argmax_tie_higher_id_loses=4)
    assert emitted_of == want, f"the cases no longer show what they are named for: {emitted_of}"


# ---- generate(speculate=k) against the plain session loop --------------------------------------------------------------------------
import logprob_cases as lc   # noqa: E402
import torch                 # noqa: E402

model_for = lc.model_for
MAX_NEW = 13   # no multiple of k + 1 for k = 1, 3, 7


def gen_inputs(B, V):
    """B = 2: the multimodal fixture prompt of the log-prob cases; otherwise text-only random ids"""
    ids, px = lc.inputs_for(B if B == 2 else 3, V)
    if B != 2:
        ids = np.random.RandomState(40 + B).randint(3, V, size=(B, 12)).astype(np.int64)
    return ids, (px.get("images"), px.get("segs"), px.get("depths"))


_REFERENCE = {}


def session_reference(eng, ids, px, K=0, fresh=False, **kw):
    """the plain session loop: a call with a log-prob request never runs in the decode pool, and its ids are the plain call's
    -> (ids [B, n], (token_logprobs, top_logprobs, top_ids)).  Computed once per (engine, inputs, arguments) and shared; fresh: run it
    again (the tests of what a call leaves behind)"""
    key = (id(eng), ids.tobytes(), K, repr(sorted(kw.items())))
    if fresh or key not in _REFERENCE:
        new = eng.generate(ids, *px, logprobs=True, top_logprobs=K, **kw)
        assert eng.last_speculation is None
        if key in _REFERENCE:
            return new, eng.last_generate_logprobs
        _REFERENCE[key] = (new, eng.last_generate_logprobs)
    new, lp = _REFERENCE[key]
    return new.copy(), tuple(a.copy() for a in lp)


def lookups(kind, truth, V, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "none":
        return None
    if kind == "truth":
        return [list(map(int, r)) for r in truth]
    if kind == "corrupted":     # every third id replaced by one that is not the truth's
        out = []
        for r in truth:
            r = list(map(int, r))
            for i in range(2, len(r), 3):
                r[i] = (r[i] + 1 + int(rng.randint(V - 2))) % V
            out.append(r)
        return out
    return [list(map(int, rng.randint(0, V, size=truth.shape[1]))) for _ in truth]


def expected_counters(ids, truth, look, k, ng, V, eos=-1):
    return np.array([simulate(list(map(int, truth[b])), [] if look is None else look[b], list(map(int, ids[b])), k, ng, V, eos)
                     for b in range(truth.shape[0])])


def check_generate(model, k, B, lookup="truth", ng=2, eos_from=None, stop_from=None, K=0, max_new=MAX_NEW):
    """ids, n_generated and log-probs array_equal to the plain session loop; the counters equal the numpy simulation.
    eos_from / stop_from: the EOS id / a 2-id stop sequence is taken from that column of row 0's greedy output."""
    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    base, _ = session_reference(eng, ids, px, max_new_tokens=max_new)
    kw = dict(max_new_tokens=max_new)
    if eos_from is not None:
        kw.update(eos_token_id=int(base[0, eos_from]), pad_token_id=0)
    if stop_from is not None:
        kw.update(stop_sequences=[[int(base[0, stop_from - 1]), int(base[0, stop_from])]], pad_token_id=0)
    ref, ref_lp = session_reference(eng, ids, px, K=K, **kw)
    look = lookups(lookup, base, V, seed=k + B)
    steps0 = eng.step_captures()
    new = eng.generate(ids, *px, speculate=k, lookup_ngram=ng, lookup_ids=look, logprobs=K > 0, top_logprobs=K, **kw)
    what = f"generate(speculate={k}) B {B} lookup {lookup} ng {ng} eos_from {eos_from} stop_from {stop_from}"
    assert new.shape == ref.shape and np.array_equal(new, ref), f"{what}: ids differ\n{new}\n{ref}"
    sp = eng.last_speculation
    assert sp is not None, f"{what}: the request was not served"
    if K > 0:
        for got, want, name in zip(eng.last_generate_logprobs, ref_lp, ("token_logprobs", "top_logprobs", "top_ids")):
            assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), f"{what}: {name} differ"
    if stop_from is None:
        full = np.where(np.arange(max_new)[None] < ref.shape[1], np.pad(ref, ((0, 0), (0, max_new - ref.shape[1]))), 0)
        want = expected_counters(ids, full, look, k, ng, V, kw.get("eos_token_id", -1))
        got = np.stack([sp["steps"], sp["tokens"], sp["drafted"], sp["accepted"]], 1)
        assert np.array_equal(got, want), f"{what}: counters {got.tolist()}, simulated {want.tolist()}"
    return sp, ref, eng.step_captures() - steps0


def check_lookup_sources(model, k, B):
    """no lookup ids, the truth, the truth with every third id replaced, random ids: the same ids each time; with the truth the loop
    takes fewer steps than tokens, and the corrupted lookup is accepted in part (what an implementation that never speculates, or
    one that accepts everything, fails)"""
    got = {}
    for kind in ("none", "truth", "corrupted", "random"):
        sp, ref, _ = check_generate(model, k, B, lookup=kind)
        got[kind] = sp
    n = ref.shape[1]
    assert (got["truth"]["steps"] < n - 1).all(), f"truth as lookup_ids: {got['truth']['steps']} steps for {n} tokens"
    assert (got["truth"]["tokens"] == n - 1).all()
    c = got["corrupted"]
    assert 0 < c["accepted"].sum() < c["drafted"].sum(), f"corrupted lookup: accepted {c['accepted']} of {c['drafted']}"
    return got


def check_logprobs(model, k=3, B=2, K=5):
    check_generate(model, k, B, lookup="truth", K=K)
    check_generate(model, k, B, lookup="corrupted", K=K, eos_from=6)


def check_streamer(model, k=3, B=2):
    """the concatenated pieces equal the returned ids, through the engine callback and through model.generate's streamer"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    base, _ = session_reference(eng, ids, px, max_new_tokens=MAX_NEW)
    for every in (1, 3):
        got = []
        new = eng.generate(ids, *px, max_new_tokens=MAX_NEW, speculate=k, lookup_ids=lookups("corrupted", base, V),
                           on_tokens=lambda first, a: got.append((first, a.copy())), stream_every=every)
        assert eng.last_speculation is not None and np.array_equal(new, base)
        assert np.array_equal(np.concatenate([a for _, a in got], 1), new)
        assert [f for f, _ in got] == list(np.cumsum([0] + [a.shape[1] for _, a in got[:-1]]))

    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got.append(v.clone())

        def end(self):
            pass

    s = Streamer()
    out = model.generate(torch.from_numpy(ids), max_new_tokens=MAX_NEW, eos_token_id=-1, streamer=s, prompt_lookup_num_tokens=k,
                         lookup_ids=lookups("truth", base, V), images=px[0], segs=px[1], depths=px[2])
    assert torch.equal(torch.stack(s.got[1:], 1), out[:, ids.shape[1]:]) and np.array_equal(out[:, ids.shape[1]:].numpy(), base)


def check_model_api(model, k=3, B=2):
    """model.generate(prompt_lookup_num_tokens=k): the same tensor, GenerateOutput.speculation filled; the default changes nothing"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=-1, images=px[0], segs=px[1], depths=px[2])
    t = torch.from_numpy(ids)
    plain = model.generate(t, output_logprobs=True, top_logprobs=3, **kw)
    assert plain.speculation is None
    look = [list(map(int, r)) for r in plain.sequences[:, ids.shape[1]:].numpy()]
    out = model.generate(t, output_logprobs=True, top_logprobs=3, prompt_lookup_num_tokens=k, max_matching_ngram_size=2, lookup_ids=look, **kw)
    assert torch.equal(out.sequences, plain.sequences) and torch.equal(out[0], plain[0])
    for name in ("token_logprobs", "top_logprobs", "top_token_ids", "sequence_logprob"):
        assert torch.equal(out[name], plain[name]), name
    assert set(out.speculation) == {"steps", "tokens", "drafted", "accepted"} and (out.speculation["steps"] < MAX_NEW - 1).all()
    bare = model.generate(t, prompt_lookup_num_tokens=k, lookup_ids=look, **kw)
    assert isinstance(bare, torch.Tensor) and torch.equal(bare, plain.sequences)


def check_not_served(model, B=2):
    """sampling, a processor set, beams, split / strict precision, a host-loop stopping criterion, B (k + 1) > 32: the output of the
    call without the argument, last_speculation None"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    t = torch.from_numpy(ids)
    kw = dict(max_new_tokens=4, eos_token_id=-1, images=px[0], segs=px[1], depths=px[2])
    base, _ = session_reference(eng, ids, px, max_new_tokens=4)
    look = lookups("truth", base, V)

    class HostCrit:   # no token-id form: the host loop
        def __call__(self, ids_, scores):
            return False

    cases = [dict(do_sample=True, temperature=0.8, top_k=20, seed=3), dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2),
             dict(num_beams=2), dict(stopping_criteria=[HostCrit()])]
    for extra in cases:
        want = model.generate(t, **kw, **extra)
        got = model.generate(t, prompt_lookup_num_tokens=3, lookup_ids=look, return_dict_in_generate=True, **kw, **extra)
        assert torch.equal(got.sequences, want), f"not served {list(extra)}: the ids differ"
        assert got.speculation is None and eng.last_speculation is None, f"not served {list(extra)}: speculation reported"
    for mode in ("split", "strict"):
        eng.set_precision(mode)
        try:
            want = eng.generate(ids, *px, max_new_tokens=4)
            got = eng.generate(ids, *px, max_new_tokens=4, speculate=3, lookup_ids=look)
            assert np.array_equal(got, want) and eng.last_speculation is None, mode
        finally:
            eng.set_precision("bf16")
    ids5, px5 = gen_inputs(5, V)     # 5 x 8 rows > 32
    want = eng.generate(ids5, *px5, max_new_tokens=4)
    got = eng.generate(ids5, *px5, max_new_tokens=4, speculate=7)
    assert np.array_equal(got, want) and eng.last_speculation is None
    got = eng.generate(ids5, *px5, max_new_tokens=4, speculate=5)   # 5 x 6 = 30 rows: served
    assert np.array_equal(got, want) and eng.last_speculation is not None


def check_refusals(model, B=2):
    """k and the n-gram size outside their ranges raise before the engine is touched; decode_step behind a speculated call refuses"""
    import pytest

    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    t = torch.from_numpy(ids)
    kw = dict(max_new_tokens=5, eos_token_id=-1, images=px[0], segs=px[1], depths=px[2])
    n0 = model._generation
    for bad in (dict(prompt_lookup_num_tokens=0), dict(prompt_lookup_num_tokens=8), dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0),
                dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=5)):
        with pytest.raises(ValueError):
            model.generate(t, **kw, **bad)
    for bad in (dict(speculate=0), dict(speculate=8), dict(speculate=2, lookup_ngram=5), dict(speculate=2, lookup_ids=[[1]] * (B + 1))):
        with pytest.raises(ValueError):
            eng.generate(ids, *px, max_new_tokens=5, **bad)
    assert model._generation == n0
    new = eng.generate(ids, *px, max_new_tokens=5, speculate=2)
    assert eng.last_speculation is not None
    with pytest.raises(RuntimeError, match="speculated"):
        eng.decode_step(new[:, -1].astype(np.int32))
    # the next prefill opens the loop again
    eng.prefill(ids, *px, has_attention_mask=True, reserve=4)
    eng.clear_attention_mask()
    eng.decode_step(new[:, 0].astype(np.int32))


def check_captures(model, B=2):
    """a second speculated call with the same B and k replays; a plain call in between adds nothing after its first; another k adds
    one; a plain generate behind a speculated one returns what it returned before"""
    eng, V = model.engine, model.config.vocab_size
    ids, px = gen_inputs(B, V)
    plain, plain_lp = session_reference(eng, ids, px, K=2, fresh=True, max_new_tokens=MAX_NEW)     # (the call's own step: captured here)
    look = lookups("corrupted", plain, V)
    eng.generate(ids, *px, max_new_tokens=MAX_NEW, speculate=3, lookup_ids=look)
    c0 = eng.step_captures()
    a = eng.generate(ids, *px, max_new_tokens=MAX_NEW, speculate=3, lookup_ids=look)
    assert eng.step_captures() == c0, "a second speculated call with the same B and k captured again"
    again, again_lp = session_reference(eng, ids, px, K=2, fresh=True, max_new_tokens=MAX_NEW)
    assert eng.step_captures() == c0, "a plain call between speculated ones captured again"
    assert np.array_equal(again, plain) and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(again_lp, plain_lp))
    b = eng.generate(ids, *px, max_new_tokens=MAX_NEW - 2, speculate=3, lookup_ids=lookups("truth", plain, V))   # other lookups, other max_new
    assert eng.step_captures() == c0 and np.array_equal(a, plain) and np.array_equal(b, plain[:, :MAX_NEW - 2])
    eng.generate(ids, *px, max_new_tokens=MAX_NEW, speculate=5, lookup_ids=look)
    assert eng.step_captures() == c0 + 1, "a different k must capture exactly one new step"
    assert np.array_equal(eng.generate(ids, *px, max_new_tokens=MAX_NEW), plain)


def check_true_dims(B, k=7, n_new=24, K=3):
    """7b dims, 2 decoder layers, the image prompt (S = 1216): ids and log-probs of a speculated call equal the plain session loop's,
    with the truth as lookup_ids"""
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
        ref = eng.generate(ids, *px, max_new_tokens=n_new, logprobs=True, top_logprobs=K)
        ref_lp = eng.last_generate_logprobs
        assert int(eng.lib.vc_last_spliced_len(eng._model)) == 1216
        new = eng.generate(ids, *px, max_new_tokens=n_new, logprobs=True, top_logprobs=K, speculate=k,
                           lookup_ids=[list(map(int, r)) for r in ref])
        sp = eng.last_speculation
        assert sp is not None, "the request was not served at 7b dims"
        assert np.array_equal(new, ref), f"7b dims B {B}: ids differ\n{new}\n{ref}"
        for got, want, name in zip(eng.last_generate_logprobs, ref_lp, ("token_logprobs", "top_logprobs", "top_ids")):
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"7b dims B {B}: {name} differ"
        assert (sp["steps"] < n_new - 1).all() and (sp["tokens"] == n_new - 1).all(), sp
        print(f"7b dims B {B} k {k}: {n_new} tokens in {sp['steps'].tolist()} verify steps, accepted {sp['accepted'].tolist()} of {sp['drafted'].tolist()}")
    finally:
        eng.close()
