"""Beam search inside the device loop (vck_beam_step, vck_kv_permute_tail, vc_generate_beam, generate(num_beams=n)): the checks shared
by the CPU-emulator tests (tests/test_beam_emu.py) and the `-m gpu` tests (tests/test_gpu_beam.py).

The reference of the kernel checks is BeamRef below: one step of `_beam_search` (vcoder_amd/model/language_model.py — HF's beam_search
and BeamSearchScorer of Transformers 4.31) restated in numpy float32, with sequences kept the way the host loop keeps them (a
[rows, length] id table permuted by beam_idx every step).  It is derived from the host loop, not from the kernel: the kernel's
back-pointer tables are checked against the id rows this restatement carries along.  The engine checks compare generate(num_beams=n)
through the device path with model._beam_search(...) on the same model; host_loop_margin() — an instrumented copy of that loop in
float64 — reports the smallest decision margin of a case, and the test asserts it is at least MIN_MARGIN, so that a fixture that
drifts towards a tie fails loudly instead of comparing noise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import e2e_cases
import kernel_cases as kc
import score_cases as sc

RS_STEP, RS_POS = 2, 3                      # csrc/kernels.h RowState
BQ_DONE, BQ_NHYP, BQ_WORST, BQ_DONE_STEP, BQ_STRIDE = 0, 1, 2, 3, 4
BP_N_EOS, BP_PAD, BP_EARLY, BP_MAXNEW, BP_EOS, BP_STRIDE = 0, 1, 2, 3, 4, 12
BH_STRIDE = 4
EARLY = {False: 0, True: 1, "never": 2}
f32 = np.float32

KERNEL_SHAPES = [(1, 1), (1, 2), (3, 5), (2, 8), (1, 16), (16, 1)]   # (B, n)
KERNEL_VOCABS = [7, 37, 32000]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _bit(x):
    return int(np.float32(x).view(np.int32))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def den_tables(T, max_new, length_penalty, len_counts_prompt, early):
    """hyp_den[step] = max(hyp_len, 1) ** length_penalty of a hypothesis added at `step` (its id row holds T + step ids) and
    done_den[step], the denominator of is_done at that step — `hyp_len`, `add_hyp`, `is_done` of _beam_search.  max_new + 1 entries:
    the open beams of the finalisation carry T + max_new ids."""
    hyp_len = lambda n_ids: n_ids if len_counts_prompt else n_ids - T
    hyp = np.array([max(hyp_len(T + s), 1) ** length_penalty for s in range(max_new + 1)], dtype=np.float64).astype(f32)
    if early == "never" and length_penalty > 0.0:
        done = np.full(max_new + 1, max(hyp_len(T + max_new), 1) ** length_penalty, dtype=np.float64).astype(f32)
    else:
        done = hyp.copy()
    return hyp, done


class BeamRef:
    """B sequences of n beams; step() is one iteration of the host loop between `topk` and `reorder_cache`, in float32."""

    def __init__(self, B, n, max_new, eos, pad, early, hyp_den, done_den, score0=None, done0=None):
        self.B, self.n, self.R, self.max_new = B, n, B * n, max_new
        self.eos, self.pad, self.early = set(int(e) for e in eos), int(pad), early
        self.hyp_den, self.done_den = np.asarray(hyp_den, f32), np.asarray(done_den, f32)
        self.score = np.zeros(self.R, f32)
        self.score[np.arange(self.R) % n != 0] = f32(-1e9)
        if score0 is not None:
            self.score = np.asarray(score0, f32).copy()
        self.hyps = [[] for _ in range(B)]          # per sequence: [score, sum, step, source row, ids]
        self.worst = [f32(1e9)] * B
        self.done = [bool(d) for d in (done0 if done0 is not None else [False] * B)]
        self.done_step = [0] * B
        self.seqs = [[] for _ in range(self.R)]     # generated ids of every row, permuted like the host loop's `seqs`
        self.tok_tab, self.parent_tab = [], []
        self.error = False
        self.events = set()

    def _add_hyp(self, b, ids_row, sum_logprobs, step, src):
        score = f32(sum_logprobs) / self.hyp_den[step]
        if len(self.hyps[b]) < self.n or score > self.worst[b]:
            self.hyps[b].append([score, f32(sum_logprobs), step, src, list(ids_row)])
            if len(self.hyps[b]) > self.n:
                srt = sorted((h[0], i) for i, h in enumerate(self.hyps[b]))
                del self.hyps[b][srt[0][1]]
                self.worst[b] = srt[1][0]
                self.events.add("evicted")
            else:
                self.worst[b] = min(score, self.worst[b])
        else:
            self.events.add("hyp_rejected")

    def step(self, cand_lp, cand_id, step):
        """cand_lp / cand_id [R, 2n]: per row its 2n best (log-prob, id), id -1 = no entry.  -> (next_tok, perm) of the step"""
        B, n, K = self.B, self.n, 2 * self.n
        ntok = np.zeros(self.R, np.int32)
        nscore = np.zeros(self.R, f32)
        nsrc = np.arange(self.R, dtype=np.int32)
        if any(self.done) and not all(self.done):
            self.events.add("done_beside_live")
        for b in range(B):
            if self.done[b]:
                ntok[b * n: b * n + n] = self.pad
                continue
            cand = []
            for row in range(b * n, b * n + n):
                for j in range(K):
                    if cand_id[row, j] >= 0:
                        cand.append((f32(cand_lp[row, j]) + self.score[row], row, int(cand_id[row, j])))
            cand.sort(key=lambda c: (-float(c[0]), c[1], c[2]))     # score descending, then the flat index beam * V + id
            scores = [c[0] for c in cand[:K]]
            if any(a == b_ and (ra != rb) for (a, ra, _), (b_, rb, _) in zip(cand[:K], cand[1:K + 1])):
                self.events.add("tie_across_beams")
            k = 0
            for rank, (sc_, src, tok) in enumerate(cand[:K]):
                if tok in self.eos:
                    if rank >= n:
                        self.events.add("eos_rank_ge_n")
                        continue
                    self.events.add("eos_rank_lt_n")
                    self._add_hyp(b, self.seqs[src], sc_, step, src)
                else:
                    nscore[b * n + k], ntok[b * n + k], nsrc[b * n + k] = sc_, tok, src
                    k += 1
                if k == n:
                    break
            if k < n:
                self.error = True
                self.events.add("error")
                ntok[b * n + k: b * n + n] = self.pad
            best = scores[0] if scores else f32(-np.inf)
            if len(self.hyps[b]) >= n:
                with np.errstate(all="ignore"):
                    if self.early is True or self.worst[b] >= best / self.done_den[step]:
                        self.done[b] = True
                        self.done_step[b] = step
                        self.events.add(f"done_{self.early}")
        self.score = nscore
        self.seqs = [self.seqs[int(nsrc[r])] + [int(ntok[r])] for r in range(self.R)]
        self.tok_tab.append(ntok.copy())
        self.parent_tab.append(nsrc.copy())
        return ntok, nsrc

    def seq_state(self):
        s = np.zeros((self.B, BQ_STRIDE), np.int32)
        h = np.zeros((self.B, self.n, BH_STRIDE), np.int32)
        for b in range(self.B):
            s[b] = [int(self.done[b]), len(self.hyps[b]), _bit(self.worst[b]), self.done_step[b]]
            for j, (score, sm, step, src, _) in enumerate(self.hyps[b]):
                h[b, j] = [_bit(score), _bit(sm), step, src]
        return s, h


def walk(tok_tab, parent_tab, step, row):
    """the ids a row holds in front of `step`, rebuilt from the back-pointer tables"""
    out = []
    for s in range(step - 1, -1, -1):
        out.append(int(tok_tab[s][row]))
        row = int(parent_tab[s][row])
    return out[::-1]


# ---- candidates ------------------------------------------------------------------------------------------------------------------
def make_cands(rng, R, n, V, pool, quant=0.0):
    """per row 2n (log-prob, id) pairs ordered as topk_logprob_kernel orders them (value descending, id ascending), ids drawn from
    `pool`; fewer than 2n when V or the pool is smaller (-inf / -1 behind them).  quant > 0: values on a grid, so that rows tie."""
    K = 2 * n
    lp = np.full((R, K), -np.inf, f32)
    ids = np.full((R, K), -1, np.int32)
    for r in range(R):
        m = min(K, V, len(pool))
        chosen = rng.choice(pool, m, replace=False)
        vals = (-np.abs(rng.randn(m)) * 2.0 - 0.01).astype(f32)
        if quant:
            vals = (np.round(vals / quant) * quant - quant).astype(f32)
        order = np.lexsort((chosen, -vals))
        lp[r, :m], ids[r, :m] = vals[order], chosen[order]
    return lp, ids


def id_pool(rng, V, size=24):
    """a small pool of vocabulary ids (the last one among them) the candidates are drawn from: EOS ids then occur at any V"""
    if V <= size:
        return np.arange(V)
    return np.unique(np.concatenate([rng.choice(V - 1, size - 1, replace=False), [V - 1]]))


# ---- vck_beam_step -----------------------------------------------------------------------------------------------------------------
class BeamDevice:
    """the kernel's buffers for B sequences of n beams and max_new steps, initialised as vc_generate_beam initialises them"""

    def __init__(self, be, B, n, max_new, eos, pad, early, hyp_den, done_den, score0=None, done0=None, pos0=5):
        self.be, self.B, self.n, self.R, self.max_new = be, B, n, B * n, max_new
        R = self.R
        self.stride = int(be.lib.vck_row_state_stride())
        score = np.zeros(R, f32)
        score[np.arange(R) % n != 0] = f32(-1e9)
        if score0 is not None:
            score = np.asarray(score0, f32)
        rows = np.zeros((R, self.stride), np.int32)
        rows[:, RS_POS] = pos0
        seq = np.zeros((B, BQ_STRIDE), np.int32)
        seq[:, BQ_WORST] = _bits(f32(1e9))
        if done0 is not None:
            seq[:, BQ_DONE] = np.asarray(done0, np.int32)
        params = np.zeros(BP_STRIDE, np.int32)
        params[BP_N_EOS], params[BP_PAD], params[BP_EARLY], params[BP_MAXNEW] = len(eos), pad, EARLY[early], max_new
        params[BP_EOS: BP_EOS + len(eos)] = eos
        self.score, self.rows, self.seq = be.f32(score), be.i32(rows), be.i32(seq)
        self.hyp = be.i32(np.zeros((B, n, BH_STRIDE), np.int32))
        self.params = be.i32(params)
        self.flags = be.i32(np.zeros(2, np.int32))
        self.next_tok = be.i32(np.full(R, -7, np.int32))
        self.perm = be.i32(np.full(R, -7, np.int32))
        self.tok_tab = be.i32(np.full((max_new, R), -7, np.int32))
        self.parent_tab = be.i32(np.full((max_new, R), -7, np.int32))
        self.hyp_den, self.done_den = be.f32(hyp_den[:max_new]), be.f32(done_den[:max_new])   # exactly max_new entries: a read behind faults

    def step(self, cand_lp, cand_id, advance=3):
        be = self.be
        kc._call(be, "vck_beam_step", be.f32(cand_lp), be.i32(cand_id), self.score, self.rows, self.next_tok, self.perm, self.tok_tab,
                 self.parent_tab, self.seq, self.hyp, self.hyp_den, self.done_den, self.params, self.flags, self.B, self.n, advance)

    def host(self, name):
        a = getattr(self, name)
        return self.be.host_f32(a) if name == "score" else self.be.host_i32(a)


def run_kernel_case(be, B, n, V, steps=5, eos_n=2, early=False, length_penalty=1.0, len_counts_prompt=True, quant=0.0, seed=0,
                    T=9, max_new=None, done0=None, cands=None, score0=None):
    """`steps` consecutive steps through the kernel and through BeamRef on the same candidates; every output compared bit for bit
    after every step, the tables as a whole at the end.  -> the restatement (its `events` say what the case exercised)"""
    rng = np.random.RandomState(seed * 1000 + B * 100 + n * 10 + V % 97)
    R = B * n
    max_new = max_new or steps
    pool = id_pool(rng, V)
    eos = [int(e) for e in rng.choice(pool, min(eos_n, len(pool)), replace=False)] if eos_n else []
    pad = int(pool[0])
    hyp_den, done_den = den_tables(T, max_new, length_penalty, len_counts_prompt, early)
    ref = BeamRef(B, n, max_new, eos, pad, early, hyp_den, done_den, score0=score0, done0=done0)
    dev = BeamDevice(be, B, n, max_new, eos, pad, early, hyp_den, done_den, score0=score0, done0=done0)
    what = f"beam_step B {B} n {n} V {V} early {early} lp {length_penalty} prompt {len_counts_prompt} quant {quant}"
    for step in range(steps):
        lp, ids = cands[step] if cands is not None else make_cands(rng, R, n, V, pool, quant)
        ntok, nsrc = ref.step(lp, ids, step)
        dev.step(lp, ids)
        w = f"{what} step {step}"
        assert np.array_equal(dev.host("next_tok"), ntok), f"{w}: next_tok {dev.host('next_tok')} expected {ntok}"
        assert np.array_equal(dev.host("perm"), nsrc), f"{w}: perm {dev.host('perm')} expected {nsrc}"
        assert np.array_equal(_bits(dev.host("score")), _bits(ref.score)), f"{w}: beam scores {dev.host('score')} expected {ref.score}"
        s, h = ref.seq_state()
        assert np.array_equal(dev.host("seq"), s), f"{w}: sequence records {dev.host('seq')} expected {s}"
        assert np.array_equal(dev.host("hyp"), h), f"{w}: hypotheses {dev.host('hyp')} expected {h}"
        assert list(dev.host("flags")) == [int(all(ref.done)), int(ref.error)], f"{w}: flags {dev.host('flags')}"
        rows = dev.host("rows")
        assert (rows[:, RS_STEP] == step + 1).all() and (rows[:, RS_POS] == 5 + step + 1).all(), f"{w}: step / position {rows[:, :4]}"
    tok, par = dev.host("tok_tab"), dev.host("parent_tab")
    assert np.array_equal(tok[:steps], np.stack(ref.tok_tab)) and np.array_equal(par[:steps], np.stack(ref.parent_tab)), f"{what}: tables"
    assert (tok[steps:] == -7).all() and (par[steps:] == -7).all(), f"{what}: wrote behind the last step"
    # the back-pointers rebuild what the host loop carries along as id rows
    for r in range(R):
        assert walk(tok, par, steps, r) == ref.seqs[r], f"{what}: row {r} rebuilt from the tables"
    for b in range(B):
        for j, (_, _, st, src, ids_row) in enumerate(ref.hyps[b]):
            assert walk(tok, par, st, src) == ids_row, f"{what}: hypothesis {j} of sequence {b} rebuilt from the tables"
    return ref


def eos_flood_cands(B, n, eos):
    """every row's two best continuations are the two EOS ids: the 2n best of a sequence are all EOS"""
    R, K = B * n, 2 * n
    lp = np.full((R, K), -np.inf, f32)
    ids = np.full((R, K), -1, np.int32)
    for r in range(R):
        lp[r, :2] = [-0.5 - 0.01 * r, -0.75 - 0.01 * r]
        ids[r, :2] = sorted(eos)
        m = min(K, 4)
        lp[r, 2:m] = [-9.0, -9.5][: m - 2]
        ids[r, 2:m] = [max(eos) + 1, max(eos) + 2][: m - 2]
    return lp, ids


def check_error_flag(be, B, n):
    """more than n EOS among the 2n best (all beams alive): the error flag is set, every token stays a vocabulary id"""
    eos = [3, 5]
    hyp_den, done_den = den_tables(9, 2, 1.0, True, False)
    score0 = np.zeros(B * n, f32)
    ref = BeamRef(B, n, 2, eos, 0, False, hyp_den, done_den, score0=score0)
    dev = BeamDevice(be, B, n, 2, eos, 0, False, hyp_den, done_den, score0=score0)
    lp, ids = eos_flood_cands(B, n, eos)
    ntok, nsrc = ref.step(lp, ids, 0)
    dev.step(lp, ids)
    assert ref.error and "error" in ref.events
    assert list(dev.host("flags")) == [int(all(ref.done)), 1], f"flags {dev.host('flags')}"
    assert np.array_equal(dev.host("next_tok"), ntok) and np.array_equal(dev.host("perm"), nsrc)
    s, h = ref.seq_state()
    assert np.array_equal(dev.host("seq"), s) and np.array_equal(dev.host("hyp"), h)


# ---- vck_kv_permute_tail -----------------------------------------------------------------------------------------------------------
PERMUTE_ROWS, PERMUTE_H, PERMUTE_HD, PERMUTE_CAP, PERMUTE_SPAN = 16, 2, 128, 48, 12


def permute_perms(R):
    cyc = np.roll(np.arange(R), 1)
    one = np.arange(R)
    one[1: R - 1] = 2                      # several rows take one parent
    out = np.arange(R)
    out[0], out[1], out[2] = R, -1, 0      # parents outside [0, R): those rows are left alone
    return {"identity": np.arange(R), "cycle": cyc, "one_parent": one, "out_of_range": out}


def check_permute_tail(be, es, R=12):
    """K and V [16][H][capS][hd * es bytes], R rows permuted over [S, pos): those positions hold the parents' bytes, every other byte
    (prompt part, dead tail, rows >= R) is unchanged, and the staging buffer is written only where a moved row needed it.  pos - S
    above the span the launch is sized for (S + 14 against 12 positions): the tail is cut at the span, as documented."""
    rng = np.random.RandomState(es)
    pb = PERMUTE_HD * es
    stride = int(be.lib.vck_row_state_stride())
    shape = (PERMUTE_ROWS, PERMUTE_H, PERMUTE_CAP, pb)
    for S in (0, 17, 33):
        for pos in (S, S + 1, S + 9, S + 14):
            end = min(pos, S + PERMUTE_SPAN)
            for name, perm in permute_perms(R).items():
                k0 = rng.randint(0, 256, size=shape).astype(np.uint8)
                v0 = rng.randint(0, 256, size=shape).astype(np.uint8)
                rows = np.zeros((R, stride), np.int32)
                rows[:, RS_POS] = pos
                d_k, d_v = be.i32(k0.view(np.int32)), be.i32(v0.view(np.int32))
                d_tmp = be.i32(np.full(2 * R * PERMUTE_H * PERMUTE_SPAN * pb // 4, 0x5A5A5A5A, np.int32))
                kc._call(be, "vck_kv_permute_tail", d_k, d_v, d_tmp, be.i32(perm.astype(np.int32)), be.i32(np.full(R, S, np.int32)),
                         be.i32(rows), R, PERMUTE_H, PERMUTE_CAP, pb, PERMUTE_SPAN)
                what = f"kv_permute_tail es {es} R {R} S {S} pos {pos} perm {name}"
                moved = [r for r in range(R) if 0 <= perm[r] < R and perm[r] != r]
                tmp = np.ascontiguousarray(be.host_i32(d_tmp)).view(np.uint8).reshape(2, R, PERMUTE_H, PERMUTE_SPAN, pb)
                for z, (got, old) in enumerate(((d_k, k0), (d_v, v0))):
                    got = np.ascontiguousarray(be.host_i32(got)).view(np.uint8).reshape(shape)
                    want = old.copy()
                    for r in moved:
                        want[r, :, S:end] = old[perm[r], :, S:end]
                    assert np.array_equal(got[:, :, S:end], want[:, :, S:end]), f"{what}: the tail does not hold the parents' rows"
                    assert np.array_equal(got, want), f"{what}: bytes outside [S, pos) or of rows outside the permutation changed"
                    for r in range(R):
                        used = end - S if r in moved else 0
                        assert (tmp[z, r, :, used:] == 0x5A).all(), f"{what}: the staging of row {r} was written behind what it needed"
                        if used:
                            assert np.array_equal(tmp[z, r, :, :used], old[perm[r], :, S:end]), f"{what}: staging of row {r}"


# ---- engine and model --------------------------------------------------------------------------------------------------------------
MIN_MARGIN = 1e-3
model_for = sc.model_for
# The tiny model's next-token distributions are nearly flat (log-probs of neighbours a few 1e-4 apart), so most prompts put SOME
# decision of an 8-step beam search closer than MIN_MARGIN to a tie.  Seeds / shapes below were chosen, while these tests were
# written, by running host_loop_margin() over candidates and keeping cases whose smallest margin is above 2e-3 on the emulator
# (printed by the test); the assertion in check_engine_case keeps them honest.
ENGINE_CASES = [
    # mode, inputs, B, n, new, seed, eos, length_penalty, early_stopping, padded mask
    ("split", "text", 2, 3, 8, 13, "none", 1.0, False, False),
    ("split", "text", 2, 3, 8, 13, "one", 1.0, False, False),
    ("split", "text", 2, 3, 8, 32, "two", 2.0, False, False),
    ("split", "text", 1, 4, 7, 13, "one", 1.0, True, False),
    ("split", "text", 2, 2, 6, 13, "one", 0.0, "never", True),
    ("split", "mm", 2, 4, 6, 0, "none", 1.0, False, False),
    ("split", "mm", 2, 2, 6, 0, "one", 1.0, False, True),
    ("bf16", "text", 2, 4, 8, 16, "one", 1.0, False, False),
    ("bf16", "mm", 2, 4, 6, 0, "none", 1.0, False, False),
    ("bf16", "mm", 1, 2, 7, 0, "one", 1.0, False, True),
]
ENGINE_CASE_FP16 = ("bf16", "text", 2, 3, 8, 13, "one", 1.0, False, False)


def engine_inputs(kind, B, V, seed):
    """-> (ids [B, T] int64, images / segs / depths kwargs).  "text": random ids, images=None; "mm": rows of the ds_img_depth_seg fixture"""
    t = lambda a: None if a is None else torch.from_numpy(a)
    if kind == "mm":
        g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs("ds_img_depth_seg")
        return ids[:B], dict(images=t(imgs[:B]), segs=t(segs[:B]), depths=t(deps[:B]))
    return np.random.RandomState(seed).randint(3, V, size=(B, 10)).astype(np.int64), dict(images=None)


def host_loop_margin(model, ids, px, n, max_new, eos_list, pad, length_penalty, early, len_counts_prompt=True, attention_mask=None):
    """An instrumented copy of model._beam_search (plain beam search: no sampling, no stopping criteria) in float64 numpy over the
    engine's own logits.  -> (sequences [B, T + L] as the host loop returns them, best scores [B], the smallest decision margin):
    the gap between the last beam a step keeps and the candidate that would be kept in its place (the n-th and (n+1)-th kept
    candidate), the gap across the rank n boundary where an EOS stands on one side of it, the distance of every `score > worst` and
    is_done comparison from its threshold, and the gap between the two best final hypotheses."""
    eng = model.engine
    B, T = ids.shape
    rep = np.repeat(np.arange(B), n)
    ex = lambda a: None if a is None else a[torch.as_tensor(rep)]
    last, _, _ = eng.prefill(ids[rep], ex(px.get("images")), ex(px.get("segs")), ex(px.get("depths")), has_attention_mask=True,
                             reserve=max_new, attention_mask=None if attention_mask is None else np.asarray(attention_mask)[rep])
    eng.clear_attention_mask()
    model._generation += 1
    V = last.shape[-1]
    eos_set = set(eos_list)
    seqs = [list(map(int, ids[b])) for b in rep]
    score = np.zeros(B * n)
    score[np.arange(B * n) % n != 0] = -1e9
    hyps, worst, done = [[] for _ in range(B)], [1e9] * B, [False] * B
    parts = {"rank": np.inf, "hyp": np.inf, "done": np.inf, "final": np.inf}
    hyp_len = lambda n_ids: n_ids if len_counts_prompt else n_ids - T

    def add_hyp(b, ids_row, s):
        sc_ = s / (max(hyp_len(len(ids_row)), 1) ** length_penalty)
        gap = abs(sc_ - worst[b]) if len(hyps[b]) >= n else np.inf     # the `score > worst` decision of a full list
        if len(hyps[b]) < n or sc_ > worst[b]:
            hyps[b].append((sc_, list(ids_row)))
            if len(hyps[b]) > n:
                srt = sorted((h[0], i) for i, h in enumerate(hyps[b]))
                del hyps[b][srt[0][1]]
                worst[b] = srt[1][0]
            else:
                worst[b] = min(sc_, worst[b])
        return gap

    logits = last.astype(np.float64)
    for step in range(max_new):
        lsm = logits - np.logaddexp.reduce(logits, axis=-1, keepdims=True)
        flat = (lsm + score[:, None]).reshape(B, n * V)
        order = np.argsort(-flat, axis=1, kind="stable")[:, : 2 * n + 1]
        ntok, nsrc, nscore = np.zeros(B * n, np.int64), np.arange(B * n), np.zeros(B * n)
        cur_len = len(seqs[0])
        for b in range(B):
            if done[b]:
                ntok[b * n: b * n + n] = pad if pad is not None else 0
                continue
            k = used = 0
            for rank in range(2 * n):
                fi = int(order[b, rank])
                tok, s, src = fi % V, float(flat[b, fi]), b * n + fi // V
                used = rank
                if tok in eos_set:
                    if rank >= n:
                        continue
                    parts["hyp"] = min(parts["hyp"], add_hyp(b, seqs[src], s))
                else:
                    nscore[b * n + k], ntok[b * n + k], nsrc[b * n + k] = s, tok, src
                    k += 1
                if k == n:
                    break
            assert k == n, "the case runs into HF's `At most n tokens can be EOS` error"
            # what a swap of neighbours in the ranking could change: the last beam kept against the next candidate that would be
            # kept in its place, and an EOS on either side of the rank n boundary (hypothesis or skipped)
            ranked = [(float(flat[b, fi]), int(fi) % V in eos_set) for fi in order[b]]
            nxt = [s_ for s_, e_ in ranked[used + 1:] if not e_]
            if nxt:
                parts["rank"] = min(parts["rank"], ranked[used][0] - nxt[0])
            if ranked[n - 1][1] != ranked[n][1]:
                parts["rank"] = min(parts["rank"], ranked[n - 1][0] - ranked[n][0])
            if len(hyps[b]) >= n:
                if early is True:
                    done[b] = True
                else:
                    hl = hyp_len(cur_len) if (early is False or length_penalty <= 0.0) else hyp_len(T + max_new)
                    thr = float(flat[b, order[b, 0]]) / (max(hl, 1) ** length_penalty)
                    if worst[b] != thr:   # (equal: the best candidate IS the worst hypothesis, the same quotient on both sides)
                        parts["done"] = min(parts["done"], abs(worst[b] - thr))
                    done[b] = worst[b] >= thr
        score = nscore
        seqs = [seqs[int(nsrc[r])] + [int(ntok[r])] for r in range(B * n)]
        if all(done) or step + 1 == max_new:
            break
        eng.reorder_cache(nsrc)
        lg, _ = eng.decode_step(ntok.astype(np.int32))
        logits = lg.astype(np.float64)
    rows, best = [], []
    for b in range(B):
        if not done[b]:
            for j in range(n):
                add_hyp(b, seqs[b * n + j], float(score[b * n + j]))
        srt = sorted(hyps[b], key=lambda h: -h[0])
        if len(srt) > 1:
            parts["final"] = min(parts["final"], srt[0][0] - srt[1][0])
        rows.append(srt[0][1])
        best.append(srt[0][0])
    L_out = min(max(len(r) for r in rows) + 1, T + max_new)
    out = np.full((B, L_out), pad if pad is not None else 0, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, : len(r)] = r
        if len(r) < L_out and eos_list:
            out[b, len(r)] = eos_list[0]
    host_loop_margin.parts = parts
    return out, np.array(best), float(min(parts.values()))


def check_engine_case(model, mode, kind, B, n, max_new, seed, eos="none", length_penalty=1.0, early=False, masked=False):
    """generate(num_beams=n) through the device path against model._beam_search(...) on the same model: equal tensors,
    sequences_scores within 1e-5 relative; the case's smallest decision margin (host_loop_margin) is asserted first.
    eos: "none"; "one": an id the best EOS-free beam of row 0 emits at step 3 (as the existing beam test picks it); "two": that id
    and a second one the beams emit."""
    eng = model.engine
    eng.set_precision(mode)
    try:
        V = model.config.vocab_size
        ids, px = engine_inputs(kind, B, V, seed)
        T = ids.shape[1]
        t_ids = torch.from_numpy(ids)
        mask = None
        if masked:
            mask = np.ones((B, T), dtype=np.int64)
            mask[-1, 1:3] = 0
        kw = dict(num_beams=n, max_new_tokens=max_new, length_penalty=length_penalty, early_stopping=early, pad_token_id=0,
                  attention_mask=None if mask is None else torch.from_numpy(mask), **px)
        eos_list = []
        if eos != "none":
            free = model.generate(t_ids, eos_token_id=-1, **kw)
            eos_list = [int(free[0, T + 2])]
            if eos == "two":
                other = [int(x) for x in free[-1, T + 1:].tolist() if int(x) != eos_list[0]]
                eos_list.append(other[0])
        what = f"beam [{mode}] {kind} B {B} n {n} new {max_new} eos {eos_list} lp {length_penalty} early {early} masked {masked}"
        ref, ref_best, margin = host_loop_margin(model, ids, px, n, max_new, eos_list, 0, length_penalty, early, attention_mask=mask)
        print(f"{what}: smallest decision margin of the host loop {margin:.3e}")
        assert margin >= MIN_MARGIN, f"{what}: the fixture's smallest decision margin {margin:.3e} is below {MIN_MARGIN}: it compares noise"
        eos_arg = -1 if not eos_list else (eos_list[0] if len(eos_list) == 1 else eos_list)
        host = model._beam_search(t_ids, px.get("images"), px.get("segs"), px.get("depths"), n, max_new, None, eos_arg, 0, kw["attention_mask"],
                                  None, length_penalty, early, True)
        assert np.array_equal(host.numpy(), ref), f"{what}: the instrumented copy of the host loop left the host loop"
        calls = []
        real = eng.generate_beam

        def spy(*a, **k):
            calls.append(1)
            return real(*a, **k)

        eng.generate_beam = spy
        try:
            out = model.generate(t_ids, eos_token_id=eos_arg, return_dict_in_generate=True, **kw)
        finally:
            del eng.generate_beam
        assert calls, f"{what}: generate(num_beams=n) did not take the device path"
        assert torch.equal(out.sequences, host), f"{what}: device path {out.sequences.tolist()}, host loop {host.tolist()}"
        got = out.sequences_scores.numpy().astype(np.float64)
        assert out.sequences_scores.dtype == torch.float32 and got.shape == (B,)
        rel = np.abs(got - ref_best) / np.abs(ref_best)
        assert (rel <= 1e-5).all(), f"{what}: sequences_scores {got}, host loop {ref_best} (relative {rel})"
        if eos_list:
            assert (out.sequences[:, T:] == eos_list[0]).any() or len(eos_list) > 1, f"{what}: the EOS never occurs"
        return out
    finally:
        eng.set_precision("bf16")


def check_prompt_rows_interchangeable(model, mode, masked):
    """The premise of the tail-only permute: the beams of a sequence are copies of one prompt row, so their prompt K / V are the
    same bits.  Seen from outside: behind a prefill of expanded rows, a full-prefix vc_reorder_cache that swaps the beams of every
    sequence leaves the logits of the next step bit-equal to those without it."""
    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = engine_inputs("mm", 2, model.config.vocab_size, 0)
        n = 3
        rep = np.repeat(np.arange(2), n)
        ex = lambda a: None if a is None else a[torch.as_tensor(rep)]
        mask = None
        if masked:
            mask = np.ones(ids.shape, dtype=np.int64)
            mask[1, 1:3] = 0
            mask = mask[rep]
        res = []
        for swap in (False, True):
            last, _, _ = eng.prefill(ids[rep], ex(px["images"]), ex(px["segs"]), ex(px["depths"]), has_attention_mask=True, reserve=4,
                                     attention_mask=mask)
            eng.clear_attention_mask()
            model._generation += 1
            for b in range(2):
                for j in range(1, n):
                    assert np.array_equal(last[b * n].view(np.int32), last[b * n + j].view(np.int32)), "prefill logits differ between beams"
            if swap:
                eng.reorder_cache(np.array([1, 2, 0, 5, 3, 4]))
            tok = np.argmax(last, -1).astype(np.int32)
            lg, _ = eng.decode_step(tok)
            res.append(lg.copy())
        assert np.array_equal(res[0].view(np.int32), res[1].view(np.int32)), \
            f"[{mode}] masked {masked}: the prompt K / V rows of a sequence's beams are not the same bits"
    finally:
        eng.set_precision("bf16")


def check_refusals(model):
    """every refusal of vc_generate_beam returns its error and leaves the engine usable: a greedy generate before and after returns
    the same ids"""
    eng = model.engine
    ids, px = engine_inputs("text", 2, model.config.vocab_size, 5)
    args = (ids, None)
    before = eng.generate(*args, max_new_tokens=5)
    import pytest

    with pytest.raises(ValueError):
        eng.generate_beam(*args, num_beams=0, max_new_tokens=4)
    with pytest.raises(ValueError):
        eng.generate_beam(*args, num_beams=9, max_new_tokens=4)          # 2 x 9 rows
    with pytest.raises(ValueError):
        eng.generate_beam(*args, num_beams=2, max_new_tokens=4, eos_token_id=list(range(3, 12)))   # 9 EOS ids
    eng.set_precision("strict")
    try:
        with pytest.raises(RuntimeError):
            eng.generate_beam(*args, num_beams=2, max_new_tokens=4)
    finally:
        eng.set_precision("bf16")
    lp = np.zeros(8, dtype=np.float32)
    eng._check(eng.lib.vc_request_generate_logprobs(eng._model, 0, lp.ctypes.data_as(C.c_void_p), None, None, C.c_size_t(8)))
    with pytest.raises(RuntimeError):
        eng.generate_beam(*args, num_beams=2, max_new_tokens=4)
    after = eng.generate(*args, max_new_tokens=5)
    assert np.array_equal(before, after)


def check_plain_graph_undisturbed(model):
    """greedy generate / a decode_step loop before and after beam calls with different n give the same ids; the second beam call
    re-captures its step for the other n"""
    eng = model.engine
    ids, px = engine_inputs("text", 2, model.config.vocab_size, 6)
    t_ids = torch.from_numpy(ids)
    greedy = lambda: model.generate(t_ids, images=None, max_new_tokens=6, eos_token_id=-1)

    def stepped():
        last, _, _ = eng.prefill(ids, None, reserve=6)
        out = [np.argmax(last, -1)]
        for _ in range(4):
            lg, nxt = eng.decode_step(None)
            out.append(np.argmax(lg, -1))
        return np.stack(out, 1)

    g0, s0 = greedy(), stepped()
    kw = dict(images=None, max_new_tokens=6, eos_token_id=-1)
    b2 = model.generate(t_ids, num_beams=2, **kw)
    b3 = model.generate(t_ids, num_beams=3, **kw)
    b2_again = model.generate(t_ids, num_beams=2, **kw)
    assert torch.equal(b2, b2_again)
    for nb, got in ((2, b2), (3, b3)):
        host = model._beam_search(t_ids, None, None, None, nb, 6, None, -1, None, None, None, 1.0, False, True)
        assert torch.equal(got, host), f"num_beams {nb}: device path {got.tolist()}, host loop {host.tolist()}"
    assert torch.equal(greedy(), g0) and np.array_equal(stepped(), s0), "a beam call disturbed the plain decode step"


def check_host_loop_routes(model):
    """do_sample, a stopping criterion and strict mode keep the host loop: the device entry point is not called"""
    eng = model.engine
    ids, _ = engine_inputs("text", 1, model.config.vocab_size, 7)
    t_ids = torch.from_numpy(ids)

    def boom(*a, **k):
        raise AssertionError("generate_beam was called")

    class Never:
        def __call__(self, ids_, scores):
            return False

    eng.generate_beam = boom
    try:
        kw = dict(images=None, num_beams=2, max_new_tokens=3, eos_token_id=-1)
        model.generate(t_ids, do_sample=True, seed=1, **kw)
        model.generate(t_ids, stopping_criteria=[Never()], **kw)
        eng.set_precision("strict")
        try:
            out = model.generate(t_ids, return_dict_in_generate=True, **kw)
            assert out.sequences_scores is not None and tuple(out.sequences_scores.shape) == (1,)
        finally:
            eng.set_precision("bf16")
        model.generate(t_ids, beam_on_device=False, **kw)     # the switch the wall-time tool uses to time the host loop
        import pytest

        with pytest.raises(AssertionError):
            model.generate(t_ids, **kw)        # the plain call does take it
    finally:
        del eng.generate_beam
