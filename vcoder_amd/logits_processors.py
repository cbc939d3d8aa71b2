"""The logits processors generate() serves (HF GenerationMixin arguments repetition_penalty, no_repeat_ngram_size, bad_words_ids,
min_length, min_new_tokens): their validation, the form the engine takes (vc_request_logits_processors) and ONE torch restatement in
the order of Transformers 4.31's `_get_logits_processor` — repetition penalty, no-repeat n-gram, bad words, min length, min new
tokens — which the host fallback loop of generate() and the host beam search apply.  The device loop runs the same processors in
logits_process_kernel (csrc/select.hip).  `apply_prefix_constraint` restates PrefixConstrainedLogitsProcessor
(generate(prefix_allowed_tokens_fn=) and, through TokenAutomaton.as_prefix_allowed_tokens_fn, generate(constraint=) on the host loops),
which 4.31 puts behind all of them.

A row's history is the caller's input_ids (image placeholders and all: HF counts the un-spliced ids) followed by the generated ids.
History ids outside [0, vocab) are skipped: HF's RepetitionPenaltyLogitsProcessor would raise an index error on the negative image
placeholders, and a banned id outside the vocabulary bans nothing."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

MAX_BAD_WORDS = 32      # what the device kernel holds (csrc/kernels.h VC_MAX_BAD_WORDS / VC_MAX_BAD_WORD_LEN / VC_MAX_EOS_EXTRA)
MAX_BAD_WORD_LEN = 8
MAX_EOS_EXTRA = 8


@dataclass
class LogitsProcessors:
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    min_length: int = 0
    bad_words_ids: List[List[int]] = field(default_factory=list)

    @property
    def active(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or self.min_new_tokens > 0 or self.min_length > 0
                or bool(self.bad_words_ids))

    def fits_device(self) -> bool:
        return len(self.bad_words_ids) <= MAX_BAD_WORDS and all(len(q) <= MAX_BAD_WORD_LEN for q in self.bad_words_ids)

    def min_new_for(self, T: int) -> int:
        """min_length folded into min_new_tokens for a prompt of T ids (both ban the EOS ids, -inf twice is -inf once)"""
        return max(int(self.min_new_tokens), int(self.min_length) - int(T), 0)


def make(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, min_length=None, bad_words_ids=None,
         eos_ids: Sequence[int] = ()) -> LogitsProcessors:
    """validates generate()'s arguments (ValueError, as HF's processors raise it) -> LogitsProcessors.  None = the default (off).
    Bad words that are exactly one EOS id are dropped, as NoBadWordsLogitsProcessor drops them."""
    import math

    p = 1.0 if repetition_penalty is None else repetition_penalty
    if not isinstance(p, (int, float)) or isinstance(p, bool) or not (p > 0) or not math.isfinite(p):
        raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {repetition_penalty}")

    def count(name, v):
        v = 0 if v is None else v
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError(f"`{name}` has to be a non-negative integer, but is {v}")
        return v

    n = count("no_repeat_ngram_size", no_repeat_ngram_size)
    m = count("min_new_tokens", min_new_tokens)
    ml = count("min_length", min_length)
    bad = []
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
        for q in bad_words_ids:
            if not isinstance(q, (list, tuple)) or len(q) == 0:
                raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists, but is {bad_words_ids}.")
            if any(not isinstance(t, int) or isinstance(t, bool) or t < 0 for t in q):
                raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
        eos = {int(e) for e in eos_ids}
        bad = [[int(t) for t in q] for q in bad_words_ids if not (len(q) == 1 and int(q[0]) in eos)]
    return LogitsProcessors(float(p), n, m, ml, bad)


@dataclass
class Guidance:
    """A classifier-free guidance request as HipEngine.generate(guidance=) / prefill_guided take it: the scale, the negative prompt's
    ids [B, Tn] (int64, rectangular, unpadded) and, when they hold placeholders, its pixels [B, 3, S, S] per modality."""
    scale: float
    negative_ids: object
    images: object = None
    segs: object = None
    depths: object = None


def check_guidance_scale(guidance_scale) -> Optional[float]:
    """generate(guidance_scale=): None or 1.0 is no request (HF's `_get_logits_processor`) -> None; else the finite scale as a float
    (ValueError otherwise)"""
    import math

    if guidance_scale is None:
        return None
    if not isinstance(guidance_scale, (int, float)) or isinstance(guidance_scale, bool) or not math.isfinite(guidance_scale):
        raise ValueError(f"`guidance_scale` has to be a finite float, but is {guidance_scale!r}")
    return None if float(guidance_scale) == 1.0 else float(guidance_scale)


def apply_guidance(cond, uncond, scale: float):
    """Classifier-free guidance, HF's UnbatchedClassifierFreeGuidanceLogitsProcessor — the FIRST processor of the list: `cond` /
    `uncond` [R, V] are the raw logits of the step behind the prompt / behind the negative prompt (both followed by the ids
    generated so far) -> scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond) in fp32, product and sum rounded
    separately: what guidance_combine_kernel (csrc/select.hip) writes in front of the other processors of the device loop.  The log
    softmax is taken in the kernel's form, (x - max) - log(sum(exp(x - max)))."""
    import torch

    def lsm(x):
        x = x.float()
        z = x - x.max(dim=-1, keepdim=True)[0]
        return z - z.exp().sum(dim=-1, keepdim=True).log()

    lc, lu = lsm(cond), lsm(uncond)
    return torch.tensor(float(scale), dtype=torch.float32) * (lc - lu) + lu


def check_warpers(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """generate(min_p=, typical_p=, epsilon_cutoff=, eta_cutoff=): validates them (ValueError, as HF's warpers raise it) ->
    (min_p, typical_p, epsilon_cutoff, eta_cutoff) as floats with 0.0 for a warper that is off — HF's GenerationConfig rules: min_p
    None or 0, typical_p None or >= 1, a cutoff None or 0."""
    def number(name, v):
        if v is None:
            return None
        if not isinstance(v, (int, float)) or isinstance(v, bool) or v != v:
            raise ValueError(f"`{name}` has to be a float, but is {v!r}")
        return float(v)

    mp, ty = number("min_p", min_p), number("typical_p", typical_p)
    ep, et = number("epsilon_cutoff", epsilon_cutoff), number("eta_cutoff", eta_cutoff)
    if mp is not None and not 0.0 <= mp <= 1.0:
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    if ty is not None and not ty > 0.0:
        raise ValueError(f"`typical_p` has to be a float > 0, but is {typical_p}")
    if ep is not None and not 0.0 <= ep < 1.0:
        raise ValueError(f"`epsilon_cutoff` has to be a float >= 0 and < 1, but is {epsilon_cutoff}")
    if et is not None and not 0.0 <= et < 1.0:
        raise ValueError(f"`eta_cutoff` has to be a float >= 0 and < 1, but is {eta_cutoff}")
    return (mp or 0.0, ty if ty is not None and ty < 1.0 else 0.0, ep or 0.0, et or 0.0)


def apply_warpers(scores, min_p: float = 0.0, typical_p: float = 0.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0,
                  min_tokens_to_keep: int = 1):
    """HF's MinPLogitsWarper -> TypicalLogitsWarper -> EpsilonLogitsWarper -> EtaLogitsWarper on `scores` [R, V] float32 (what
    temperature, top-k and top-p left; removed entries -inf), each over the survivors of the one in front of it; arguments as
    check_warpers returns them (0.0: off).  -> a new tensor with the removed entries at -inf.  What the host sampling loops apply
    behind their top-p (min_tokens_to_keep 1) and beam-sample applies with min_tokens_to_keep = 2; the device sampler restates it
    in warp_thresholds (csrc/select.hip)."""
    import torch

    ninf = float("-inf")
    out = scores.float().clone()
    keep_n = max(1, min(int(min_tokens_to_keep), out.shape[-1]))

    def entropy(x):
        lp = torch.log_softmax(x, dim=-1)
        return -(lp * lp.exp()).nansum(dim=-1, keepdim=True), lp

    def under_kth(x):   # the cutoffs spare every score that reaches the keep_n-th largest
        return x < torch.topk(x, keep_n, dim=-1)[0][..., -1:]

    if min_p > 0.0:
        p = torch.softmax(out, dim=-1)
        remove = p < min_p * p.amax(dim=-1, keepdim=True)
        first = torch.argsort(out, dim=-1, descending=True)[..., :keep_n]
        remove.scatter_(-1, first, False)
        out = out.masked_fill(remove, ninf)
    if 0.0 < typical_p < 1.0:
        H, lp = entropy(out)
        s, order = torch.sort((-lp - H).abs(), dim=-1, descending=False)
        cum = out.gather(-1, order).softmax(dim=-1).cumsum(dim=-1)
        last = (cum < typical_p).sum(dim=-1, keepdim=True).clamp_(max=out.shape[-1] - 1)
        remove_sorted = s > s.gather(-1, last)
        remove_sorted[..., :keep_n] = False
        out = out.masked_fill(torch.zeros_like(remove_sorted).scatter_(-1, order, remove_sorted), ninf)
    if epsilon_cutoff > 0.0:
        out = out.masked_fill((torch.softmax(out, dim=-1) < epsilon_cutoff) & under_kth(out), ninf)
    if eta_cutoff > 0.0:
        H, _ = entropy(out)
        e = torch.tensor(float(eta_cutoff), dtype=torch.float32)
        eta = torch.minimum(e, torch.sqrt(e) * torch.exp(-H))
        out = out.masked_fill((torch.softmax(out, dim=-1) < eta) & under_kth(out), ninf)
    return out


def apply_torch(proc: LogitsProcessors, history, scores, prompt_len: int, eos_ids: Sequence[int]):
    """`scores` [R, V] float32 of the next token behind `history` [R, L] int64 (prompt_len prompt ids, then the generated ones)
    -> the processed scores (a new tensor).  HF 4.31's order; fp32 arithmetic (the penalty's division is torch's IEEE division)."""
    import torch

    out = scores.clone()
    R, V = out.shape
    L = history.shape[1]
    hist = [[int(t) for t in row] for row in history.tolist()]
    if proc.repetition_penalty != 1.0:
        for r in range(R):
            ids = sorted({t for t in hist[r] if 0 <= t < V})
            if not ids:
                continue
            idx = torch.tensor(ids, dtype=torch.long)
            s = scores[r, idx]
            out[r, idx] = torch.where(s < 0, s * proc.repetition_penalty, s / proc.repetition_penalty)
    ninf = float("-inf")
    n = proc.no_repeat_ngram_size
    if n > 0 and L + 1 >= n:
        for r in range(R):
            h = hist[r]
            tail = h[L - n + 1:] if n > 1 else []
            for i in range(L - n + 1):
                if h[i:i + n - 1] == tail and 0 <= h[i + n - 1] < V:
                    out[r, h[i + n - 1]] = ninf
    for q in proc.bad_words_ids:
        if not 0 <= q[-1] < V:
            continue
        pre = q[:-1]
        for r in range(R):
            if not pre or (len(pre) <= L and hist[r][L - len(pre):] == pre):
                out[r, q[-1]] = ninf
    eos = [int(e) for e in eos_ids if 0 <= int(e) < V]
    if eos and (L < proc.min_length or L - prompt_len < proc.min_new_tokens):
        out[:, eos] = ninf
    return out


def apply_prefix_constraint(fn, history, scores, num_beams: int = 1, skip=None):
    """HF 4.31's PrefixConstrainedLogitsProcessor: row r of `scores` [R, V] keeps its value at the ids
    fn(r // num_beams, history[r]) returns and is -inf elsewhere; an empty list leaves the row all -inf.  Ids outside [0, V) allow
    nothing (HF would raise an index error).  Rows where `skip` [R] is true — finished rows, whose token is pad whatever their
    scores are — are returned as they came.  -> a new tensor."""
    import torch

    R, V = scores.shape
    out = torch.full_like(scores, float("-inf"))
    for r in range(R):
        if skip is not None and bool(skip[r]):
            out[r] = scores[r]
            continue
        ids = [int(t) for t in fn(r // num_beams, history[r])]
        ids = [t for t in ids if 0 <= t < V]
        if ids:
            idx = torch.tensor(ids, dtype=torch.long)
            out[r, idx] = scores[r, idx]
    return out
