"""Shared checks of the sampler's further warpers — min_p, typical_p, epsilon_cutoff, eta_cutoff behind temperature / top-k / top-p
(csrc/select.hip warp_thresholds; vc_request_sampling_warpers; generate(min_p=, typical_p=, epsilon_cutoff=, eta_cutoff=)) — used by
tests/test_warpers_emu.py (CPU emulator) and tests/test_gpu_warpers.py (MI355X):

  1. a float64 numpy restatement of the whole chain and the torch restatement logits_processors.apply_warpers against Transformers'
     classes applied in sequence;
  2. the kept mask vck_warp_support writes against the restatement, between the chain with every threshold tightened and loosened
     by 2e-3 (the device compares fp32 block-ordered sums: a token on a boundary may fall on either side);
  3. draws of vck_spec_select: repeatable, inside the probe's mask, distributed as the restatement's softmax;
  4. generate() on the tiny models, compared id for id where one token survives the warpers (the device and the host draw from
     different streams), and against the host restatement's support at the usual settings."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

import kernel_cases as kc
import logits_processor_cases as pc
from vcoder_amd import logits_processors as lp

RS = kc.RS
RS_MINP, RS_TYPICAL, RS_EPS, RS_ETA = 114, 115, 116, 117   # csrc/kernels.h RowStateField

# (T, top_k, top_p, min_p, typical, eps, eta); 0: off (top_p: 1)
SETTINGS = {
    "typ": (1.0, 0, 1.0, 0.0, 0.9, 0.0, 0.0),
    "typ_tight": (1.0, 0, 1.0, 0.0, 0.2, 0.0, 0.0),
    "k_p_typ": (0.7, 50, 0.95, 0.0, 0.8, 0.0, 0.0),
    "minp": (1.0, 0, 1.0, 0.05, 0.0, 0.0, 0.0),
    "cli": (0.2, 50, 1.0, 0.1, 0.0, 0.0, 0.0),
    "eps": (1.0, 0, 1.0, 0.0, 0.0, 3e-4, 0.0),
    "eta": (1.0, 0, 1.0, 0.0, 0.0, 0.0, 2e-3),
    "all": (0.9, 200, 0.98, 0.02, 0.95, 1e-3, 2e-3),
}
SIZES = (96, 4100, 32000)
BAND = 2e-3


def setting(name, V):
    T, k, p, mp, ty, ep, et = SETTINGS[name]
    if V == 96:   # the cutoffs of a small vocabulary
        ep, et = (0.02 if ep else 0.0), (0.05 if et else 0.0)
    return T, k, p, mp, ty, ep, et


def logits_row(V):
    return (np.random.RandomState(5).randn(V) * 1.5).astype(np.float32)


# ---- 1. restatements ------------------------------------------------------------------------------------------------------------
def _probs(z):
    e = np.where(np.isfinite(z), np.exp(z - z[np.isfinite(z)].max()), 0.0)
    return e / e.sum()


def _entropy(p):
    q = p[p > 0]
    return float(-(q * np.log(q)).sum())


def ref_chain(lg, T=1.0, top_k=0, top_p=1.0, min_p=0.0, typical=0.0, eps=0.0, eta=0.0):
    """temperature -> top-k -> top-p -> min-p -> typical -> epsilon -> eta with min_tokens_to_keep = 1, float64; -> the warped row
    (removed entries -inf).  Every warper sees the survivors of those in front of it."""
    z = lg.astype(np.float64) / T
    V = z.shape[-1]
    if top_k and 0 < top_k < V:
        z = np.where(z < np.sort(z)[-top_k], -np.inf, z)
    if top_p < 1.0:
        order = np.argsort(z, kind="stable")
        remove = np.cumsum(_probs(z)[order]) <= (1.0 - top_p)
        remove[-1] = False
        z = z.copy()
        z[order[remove]] = -np.inf
    if min_p > 0.0:
        p = _probs(z)
        z = np.where((p < min_p * p.max()) & (z < z.max()), -np.inf, z)
    if 0.0 < typical < 1.0:
        p = _probs(z)
        with np.errstate(divide="ignore"):
            s = np.abs(-np.log(p) - _entropy(p))
        order = np.argsort(s, kind="stable")
        last = min(int((np.cumsum(p[order]) < typical).sum()), V - 1)
        z = np.where(s > s[order[last]], -np.inf, z)
    if eps > 0.0:
        z = np.where((_probs(z) < eps) & (z < z.max()), -np.inf, z)
    if eta > 0.0:
        p = _probs(z)
        thr = min(eta, np.sqrt(eta) * np.exp(-_entropy(p)))
        z = np.where((p < thr) & (z < z.max()), -np.inf, z)
    return z


def ref_band(lg, T, top_k, top_p, min_p, typical, eps, eta):
    """-> (S-, S+, S): the kept sets of the chain with every threshold that is on tightened / loosened by BAND, and as given"""
    tight = ref_chain(lg, T, top_k, top_p - BAND if top_p < 1.0 else 1.0, min_p * (1 + BAND), typical * (1 - BAND), eps * (1 + BAND),
                      eta * (1 + BAND))
    loose = ref_chain(lg, T, top_k, min(1.0, top_p + BAND), min_p * (1 - BAND), min(typical * (1 + BAND), 1.0 - 1e-12) if typical else 0.0,
                      eps * (1 - BAND), eta * (1 - BAND))
    return np.isfinite(tight), np.isfinite(loose), np.isfinite(ref_chain(lg, T, top_k, top_p, min_p, typical, eps, eta))


def hf_chain(lg, T, top_k, top_p, min_p, typical, eps, eta, min_tokens_to_keep=1, head=True):
    """Transformers' warpers in GenerationMixin's order on a [R, V] float32 tensor; head=False: only the four behind top-p"""
    from transformers.generation import logits_process as hf

    x = torch.as_tensor(lg, dtype=torch.float32).reshape(-1, lg.shape[-1]).clone()
    ids = torch.zeros((x.shape[0], 1), dtype=torch.long)
    m = dict(min_tokens_to_keep=min_tokens_to_keep)
    ws = []
    if head:
        ws.append(hf.TemperatureLogitsWarper(float(T)))
        if top_k:
            ws.append(hf.TopKLogitsWarper(int(top_k), **m))
        if top_p < 1.0:
            ws.append(hf.TopPLogitsWarper(float(top_p), **m))
    if min_p > 0.0:
        ws.append(hf.MinPLogitsWarper(float(min_p), **m))
    if 0.0 < typical < 1.0:
        ws.append(hf.TypicalLogitsWarper(float(typical), **m))
    if eps > 0.0:
        ws.append(hf.EpsilonLogitsWarper(float(eps), **m))
    if eta > 0.0:
        ws.append(hf.EtaLogitsWarper(float(eta), **m))
    for w in ws:
        x = w(ids, x)
    return x


def check_restatement_against_hf():
    """the float64 restatement keeps exactly what Transformers' classes, applied in sequence in fp32, keep — in all 24 cases — and the
    band S+ \\ S- around it stays a hair: max(1, 2 %) of the kept set"""
    shares = []
    for V in SIZES:
        lg = logits_row(V)
        for name in SETTINGS:
            st = setting(name, V)
            lo, hi, mid = ref_band(lg, *st)
            got = torch.isfinite(hf_chain(lg, *st)[0]).numpy()
            assert np.array_equal(got, mid), f"{name} V {V}: Transformers keeps {got.sum()}, the restatement {mid.sum()}; differ at {np.nonzero(got != mid)[0][:8]}"
            assert (lo <= mid).all() and (mid <= hi).all(), f"{name} V {V}: the band does not enclose the chain"
            n = int((hi & ~lo).sum())
            shares.append((n / max(int(hi.sum()), 1), n, int(hi.sum()), name, V))
            assert n <= max(1, 0.02 * hi.sum()), f"{name} V {V}: band of {n} tokens around {hi.sum()} kept"
    print("bands:", sorted(shares)[-3:], "largest", max(shares, key=lambda t: t[1]))


def check_torch_restatement_against_hf(seed=0, V=157, rows=6):
    """logits_processors.apply_warpers == Transformers' four classes in sequence, bit for bit, at min_tokens_to_keep 1 and 2, on rows
    that already hold -inf entries (what top-k left) and on peaked rows where the cutoffs would remove everything but the maximum"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(rows, V) * 2.0).astype(np.float32)
    x[1, rng.choice(V, V - 3, replace=False)] = -np.inf
    x[2, 7] = 40.0
    x[3, rng.choice(V, V // 2, replace=False)] = -np.inf
    xt = torch.from_numpy(x)
    n = 0
    for mtk in (1, 2):
        for mp, ty, ep, et in ((0.05, 0, 0, 0), (1.0, 0, 0, 0), (0, 0.9, 0, 0), (0, 0.2, 0, 0), (0, 1e-4, 0, 0), (0, 0, 0.02, 0), (0, 0, 0.999, 0),
                               (0, 0, 0, 0.05), (0, 0, 0, 0.9), (0.02, 0.95, 0.01, 0.02), (0.3, 0.5, 0.2, 0.3)):
            want = hf_chain(x, 1.0, 0, 1.0, mp, ty, ep, et, min_tokens_to_keep=mtk, head=False)
            got = lp.apply_warpers(xt, float(mp), float(ty), float(ep), float(et), min_tokens_to_keep=mtk)
            assert torch.equal(got, want), f"apply_warpers({mp}, {ty}, {ep}, {et}, keep {mtk}): kept {torch.isfinite(got).sum(1).tolist()}, " \
                                           f"Transformers {torch.isfinite(want).sum(1).tolist()}"
            assert int(torch.isfinite(got).sum(1).min()) >= min(mtk, 1)
            n += int((torch.isfinite(got) != torch.isfinite(xt)).any())
    assert n >= 16, "the settings remove nothing: the case shows nothing"
    assert torch.equal(lp.apply_warpers(xt), xt) and lp.apply_warpers(xt) is not xt


def check_validation():
    assert lp.check_warpers() == (0.0, 0.0, 0.0, 0.0)
    assert lp.check_warpers(0, 1.0, 0.0, None) == (0.0, 0.0, 0.0, 0.0) and lp.check_warpers(None, 2.5) == (0.0, 0.0, 0.0, 0.0)
    assert lp.check_warpers(0.05, 0.9, 3e-4, 2e-3) == (0.05, 0.9, 3e-4, 2e-3) and lp.check_warpers(1, 1e-4)[:2] == (1.0, 1e-4)
    for kw in (dict(min_p=-0.1), dict(min_p=1.5), dict(typical_p=0), dict(typical_p=-1.0), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1),
               dict(eta_cutoff=1.0), dict(eta_cutoff=-1e-3), dict(min_p="0.1"), dict(typical_p=float("nan")), dict(eta_cutoff=True)):
        try:
            lp.check_warpers(**kw)
            raise AssertionError(f"check_warpers({kw}) was accepted")
        except ValueError:
            pass


# ---- 2. the kept mask of the kernel ---------------------------------------------------------------------------------------------
def warp_rows(settings, **fields):
    """RowState records, one per (T, top_k, top_p, min_p, typical, eps, eta)"""
    n = len(settings)
    rows = kc.make_rows(n, MAXNEW=1, SAMPLE=1, OUT_OFF=list(range(n)), **fields)
    for r, (T, k, p, mp, ty, ep, et) in enumerate(settings):
        rows[r, RS["INVTEMP"]] = kc._f32_bits(1.0 / T)
        rows[r, RS["TOPK"]] = k
        rows[r, RS["TOPP"]] = kc._f32_bits(p)
        for f, v in ((RS_MINP, mp), (RS_TYPICAL, ty), (RS_EPS, ep), (RS_ETA, et)):
            rows[r, f] = kc._f32_bits(v)
    return rows


def support(be, lg, rows, lds, ldl=None):
    """one launch of vck_warp_support over logits [n, V] (ldl 0: every record reads row 0) -> keep [n, V] bool"""
    n, V = rows.shape[0], lg.shape[-1]
    lgd, rd = be.f32(lg), be.i32(rows)
    keep = be.i32(np.full((n, V), -7))
    be.lib.vck_warp_support(be.ptr(lgd), V if ldl is None else ldl, V, be.ptr(rd), n, be.ptr(keep), lds, None)
    be.sync()
    k = be.host_i32(keep)
    assert ((k == 0) | (k == 1)).all(), "vck_warp_support left entries unwritten"
    assert np.array_equal(be.host_i32(rd), rows), "vck_warp_support wrote a record"
    return k.astype(bool)


def check_kept_mask(be, V, lds):
    """the eight settings as eight different records of ONE launch over the same row: S- <= mask <= S+ for each (the band asserted a
    hair first); a ninth record with all four off keeps what a record of the same top-k / top-p with cleared words keeps"""
    lg = logits_row(V)
    names = list(SETTINGS)
    sts = [setting(n, V) for n in names]
    off = (0.7, 50, 0.95, 0.0, 0.0, 0.0, 0.0)
    rows = warp_rows(sts + [off, (0.7, 50, 0.95, 0.0, 1.0, 0.0, 0.0)])
    mask = support(be, lg, rows, lds, ldl=0)
    for r, name in enumerate(names):
        lo, hi, _ = ref_band(lg, *sts[r])
        n = int((hi & ~lo).sum())
        assert n <= max(1, 0.02 * hi.sum()), f"{name} V {V}: band of {n} tokens around {hi.sum()} kept"
        print(f"{name} V {V} lds {lds}: kept {int(mask[r].sum())} in [{int(lo.sum())}, {int(hi.sum())}]")
        assert (mask[r] >= lo).all(), f"{name} V {V} lds {lds}: removed {np.nonzero(lo & ~mask[r])[0][:8]} of the tightened set ({mask[r].sum()} kept, {lo.sum()} .. {hi.sum()})"
        assert (mask[r] <= hi).all(), f"{name} V {V} lds {lds}: kept {np.nonzero(mask[r] & ~hi)[0][:8]} outside the loosened set ({mask[r].sum()} kept, {lo.sum()} .. {hi.sum()})"
    lo, hi, _ = ref_band(lg, *off)
    assert (mask[8] >= lo).all() and (mask[8] <= hi).all() and 0 < mask[8].sum() <= 50, "all four off: not the top-k / top-p set"
    assert np.array_equal(mask[9], mask[8]), "typical_p = 1.0 is not off"
    return mask


def check_survivor_rows(be, V, lds):
    """rows removed down to -inf in front of the warpers: typical over a 1-survivor set keeps it, over a 2-survivor set (p = .7 / .3)
    keeps the likelier token at mass .5 and both at mass .9; min-p / epsilon / eta over them keep the maximum"""
    lg = np.full((5, V), -np.inf, dtype=np.float32)
    a, b = V // 3, V - 2
    lg[0, a] = 1.25
    lg[1:, a], lg[1:, b] = np.float32(np.log(0.7)), np.float32(np.log(0.3))
    sts = [(1.0, 0, 1.0, 0.0, 0.5, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 0.5, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 0.9, 0.0, 0.0),
           (1.0, 0, 1.0, 0.5, 0.0, 0.0, 0.0), (0.5, 0, 1.0, 0.0, 0.99, 0.2, 0.3)]
    mask = support(be, lg, warp_rows(sts), lds)
    for r, st in enumerate(sts):
        want = np.isfinite(ref_chain(lg[r], *st))
        assert np.array_equal(mask[r], want), f"row {r} V {V} lds {lds}: kept {np.nonzero(mask[r])[0]}, the restatement {np.nonzero(want)[0]}"
    assert mask.sum(1).tolist() == [1, 1, 2, 1, 1]


# ---- 3. draws -------------------------------------------------------------------------------------------------------------------
def check_draws(be, V, name, draws=2048, seed0=1234):
    """vck_spec_select over `draws` records of one setting that differ in their seed (one launch; every record reads the same row):
    the same seeds give the same ids, in the staged and in the global-memory form alike; every draw lies in the mask the probe
    returned; the total variation against the restatement's softmax stays under check_sampling's bound (4 x the multinomial noise)"""
    lg = logits_row(V)
    st = setting(name, V)
    rows = warp_rows([st] * draws, SEED_HI=77)
    rows[:, RS["SEED_LO"]] = [(seed0 + 7919 * r) & 0x7FFFFFFF for r in range(draws)]
    lgd, rd, nq = be.f32(lg), be.i32(rows), be.i32(np.ones(draws))
    got = {}
    for lds in (-1, 0, -1):
        sel = be.i32(np.full(draws, -1))
        be.lib.vck_spec_select(be.ptr(lgd), 0, V, be.ptr(rd), be.ptr(nq), be.ptr(sel), draws, 1, lds, None)
        be.sync()
        ids = be.host_i32(sel).copy()
        assert all(np.array_equal(ids, g) for g in got.values()), f"{name} V {V}: lds_floats {lds} draws other ids under the same seeds"
        got[lds] = ids
        mask = support(be, lg, rows[:1], lds)[0]
        assert mask[ids].all(), f"{name} V {V} lds {lds}: draws {ids[~mask[ids]][:8]} lie outside the probe's mask"
    ids = got[-1]
    probs = _probs(ref_chain(lg, *st))
    counts = np.bincount(ids, minlength=V)
    tv = 0.5 * np.abs(counts / draws - probs).sum()
    bound = 4.0 * np.sqrt(probs * (1 - probs) / (2 * np.pi * draws)).sum() + 1e-3
    print(f"{name} V {V}: {len(set(ids.tolist()))} distinct ids of {int((probs > 0).sum())}, total variation {tv:.4f}, bound {bound:.4f}")
    assert tv < bound, f"{name} V {V}: total variation {tv:.4f} > {bound:.4f}"
    if (probs > 0).sum() > 4:
        rows2 = rows.copy()
        rows2[:, RS["STEP"]] = 1
        sel, rd2 = be.i32(np.full(draws, -1)), be.i32(rows2)
        be.lib.vck_spec_select(be.ptr(lgd), 0, V, be.ptr(rd2), be.ptr(nq), be.ptr(sel), draws, 1, -1, None)
        be.sync()
        assert not np.array_equal(be.host_i32(sel), ids), "the step counter must change the draw"


def check_selection_at_32000(be):
    """one launch of the selection at the true vocabulary size, all four warpers on, both forms: inside the probe's mask"""
    V, n = 32000, 8
    lg = logits_row(V)
    st = setting("all", V)
    rows = warp_rows([st] * n, SEED_HI=3, SEED_LO=list(range(100, 100 + n)))
    out = be.zeros((n, 1), "i32")
    nxt = kc._select(be, np.tile(lg, (n, 1)), rows, out, 64, V, None, advance=0)[0]
    mask = support(be, lg, rows[:1], -1)[0]
    assert mask[nxt].all() and len(set(nxt.tolist())) > 1, f"V 32000: draws {nxt} outside the mask or all alike"
    sel, lgd, rd, nq = be.i32(np.full(n, -1)), be.f32(lg), be.i32(rows), be.i32(np.ones(n))   # (alive until the launch is through)
    be.lib.vck_spec_select(be.ptr(lgd), 0, V, be.ptr(rd), be.ptr(nq), be.ptr(sel), n, 1, 0, None)
    be.sync()
    assert np.array_equal(be.host_i32(sel), nxt), "the global-memory form selects other ids than vck_select_embed"


# ---- 4. model level -------------------------------------------------------------------------------------------------------------
N_NEW = 6
_models = {}
TEMP = 0.9
USUAL = dict(do_sample=True, temperature=TEMP, top_k=30, top_p=0.95, seed=11)
WARP = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=2e-3, eta_cutoff=5e-3)
inputs_for = pc.inputs_for


def model_for(variant="vcoder_ds", lib=None, operands="bf16", seed=42):
    """one model per (variant, library) for the tests of this feature alone, released by close_models() (as constraint_cases.model_for)"""
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


def _host(model, V):
    """kwargs that send a call to the host sampling loop without changing its scores: a callable that allows every id"""
    every = list(range(V))
    return dict(prefix_allowed_tokens_fn=lambda b, ids: every)


def host_rows(model, ids, px, new):
    """the raw rows [n][B, V] of the host loop's primitives, teacher-forced with the ids `new` [B, n]"""
    eng = model.engine
    last, _, _ = eng.prefill(ids, px["images"], px["segs"], px["depths"], has_attention_mask=True, reserve=new.shape[1])
    eng.clear_attention_mask()
    rows = [torch.from_numpy(last).float()]
    for s_ in range(new.shape[1] - 1):
        rows.append(torch.from_numpy(eng.decode_step(np.ascontiguousarray(new[:, s_], dtype=np.int32))[0]).float())
    return rows


def check_single_survivor(model, mode, B):
    """where the warpers leave one token the sampled call is decided: min_p = 1.0 and epsilon_cutoff = 0.999 (top_k 0, T 0.9) return
    the greedy ids; typical_p = 1e-4 returns the per-step most typical token of the host's logits — on the device loop and on the
    host loop alike — which is not the greedy token at some step.  An engine that swallows the arguments samples freely there."""
    from vcoder_amd.model import language_model as lm

    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T, V = ids.shape[1], model.config.vocab_size
        greedy = _gen(model, ids, px)
        skw = dict(do_sample=True, temperature=TEMP, top_k=0, seed=5)
        free = _gen(model, ids, px, **skw)
        assert not torch.equal(free, greedy), "the free sampled call returns the greedy ids: the case shows nothing"
        for kw in (dict(min_p=1.0), dict(epsilon_cutoff=0.999)):
            dev = _gen(model, ids, px, **skw, **kw)
            assert torch.equal(dev, greedy), f"[{mode}] B {B} {kw}: device loop {dev[:, T:].tolist()}, greedy {greedy[:, T:].tolist()}"
            host = _gen(model, ids, px, **skw, **kw, **_host(model, V))
            assert torch.equal(host, greedy), f"[{mode}] B {B} {kw}: host loop {host[:, T:].tolist()}, greedy {greedy[:, T:].tolist()}"
        dev = _gen(model, ids, px, **skw, typical_p=1e-4)
        host = _gen(model, ids, px, **skw, typical_p=1e-4, **_host(model, V))
        new = dev[:, T:].numpy()
        want = []
        for sc in host_rows(model, ids, px, new):
            lsm = torch.log_softmax(sc / TEMP, dim=-1)
            H = -(lsm * lsm.exp()).nansum(-1, keepdim=True)
            want.append((-lsm - H).abs().argmin(-1))
        want = torch.stack(want, 1)
        print(f"[{mode}] B {B}: greedy {greedy[:, T:].tolist()} most typical {want.tolist()}")
        assert torch.equal(dev[:, T:], want), f"[{mode}] B {B} typical_p=1e-4: device loop {new.tolist()}, most typical {want.tolist()}"
        assert torch.equal(host, dev), f"[{mode}] B {B} typical_p=1e-4: host loop {host[:, T:].tolist()}, device loop {new.tolist()}"
        assert not torch.equal(dev, greedy), "the most typical token is the greedy one at every step: the case shows nothing"
        # a greedy call applies no warper (HF's rule), but validates
        assert torch.equal(_gen(model, ids, px, min_p=0.3, typical_p=0.2, epsilon_cutoff=0.5, eta_cutoff=0.5), greedy)
    finally:
        eng.set_precision("bf16")


def check_usual_settings(model, mode, B, seeds=(11, 12, 13)):
    """temperature 0.9, top_k 30, top_p 0.95 with all four warpers on: the call repeats under its seed, and every id lies in the
    loosened kept set S+ of the host restatement (HF's order, every threshold loosened by 2e-3) of that step's host scores"""
    from vcoder_amd.model import language_model as lm

    eng = model.engine
    eng.set_precision(mode)
    try:
        ids, px = inputs_for(B)
        T = ids.shape[1]
        seen = set()
        for seed in seeds:
            kw = dict(USUAL, seed=seed, **WARP)
            out = _gen(model, ids, px, **kw)
            assert torch.equal(out, _gen(model, ids, px, **kw)), "a sampled call does not repeat under its seed"
            new = out[:, T:].numpy()
            for s_, sc in enumerate(host_rows(model, ids, px, new)):
                sc = sc / TEMP
                kth = torch.topk(sc, USUAL["top_k"])[0][..., -1, None]
                kept = lm._top_p_filter(sc.masked_fill(sc < kth, float("-inf")), USUAL["top_p"] + BAND)
                kept = lp.apply_warpers(kept, WARP["min_p"] * (1 - BAND), WARP["typical_p"] * (1 + BAND), WARP["epsilon_cutoff"] * (1 - BAND),
                                        WARP["eta_cutoff"] * (1 - BAND))
                for b in range(B):
                    assert bool(torch.isfinite(kept[b, int(new[b, s_])])), \
                        f"[{mode}] seed {seed} row {b} step {s_}: id {int(new[b, s_])} lies outside the warped support ({int(torch.isfinite(kept[b]).sum())} kept)"
                    seen.add((b, s_, int(new[b, s_])))
        assert len(seen) > B * N_NEW, "every seed drew the same ids: the sampler is not exercised"
    finally:
        eng.set_precision("bf16")


def check_combinations(model, B=2):
    """the warpers beside what else selects through the same body — decided (min_p = 1.0: the sampled call must return the greedy
    call's ids) and at the usual settings (repeatable): the five processors, constraint=, guidance, log-probs (those of the raw rows:
    the greedy call's), num_return_sequences in both forms, speculation under speculate_selection="any" (array_equal to the call
    without it)"""
    from vcoder_amd.constraints import TokenAutomaton

    eng = model.engine
    ids, px = inputs_for(B)
    T, V = ids.shape[1], model.config.vocab_size
    plain = _gen(model, ids, px)
    one = dict(do_sample=True, temperature=TEMP, top_k=0, seed=5, min_p=1.0)
    usual = dict(USUAL, **WARP)
    used = {int(t) for t in plain[:, T:].reshape(-1)}
    A = [t for t in range(7, V) if t not in used][:: max((V - 7 - len(used)) // 8, 1)][:8]
    a = TokenAutomaton.from_sequences([[A[0], A[1], A[2]], [A[0], A[3]], [A[4], A[4], A[4], A[4]]], [A[5]])
    for what, kw in (("processors", pc.configs_from(plain, T)["all_five"][0]), ("constraint", dict(constraint=a, eos_token_id=A[5], pad_token_id=0)),
                     ("guidance", dict(guidance_scale=1.5))):
        base = _gen(model, ids, px, **kw)
        got = _gen(model, ids, px, **kw, **one)
        assert torch.equal(got, base), f"{what}: sampled with min_p = 1.0 {got[:, T:].tolist()}, greedy {base[:, T:].tolist()}"
        u = _gen(model, ids, px, **kw, **usual)
        assert torch.equal(u, _gen(model, ids, px, **kw, **usual)), f"{what}: the call does not repeat under its seed"
        if what == "guidance":
            assert eng.last_guidance is not None
    lkw = dict(output_logprobs=True, top_logprobs=3)
    base, got = _gen(model, ids, px, **lkw), _gen(model, ids, px, **lkw, **one)
    assert torch.equal(got.sequences, base.sequences) and torch.equal(got.top_token_ids, base.top_token_ids)
    assert np.array_equal(got.token_logprobs.numpy().view(np.int32), base.token_logprobs.numpy().view(np.int32)), "the log-probs are not those of the raw rows"
    for fan in (False, True):
        two = _gen(model, ids, px, num_return_sequences=2, fan_out=fan, **one)
        assert torch.equal(two, plain[np.repeat(np.arange(B), 2)]), f"num_return_sequences fan_out {fan}: not the greedy rows twice"
        u = _gen(model, ids, px, num_return_sequences=2, fan_out=fan, **usual)
        rep = np.repeat(np.arange(B), 2)
        want = _gen(model, ids[rep], {k: (None if v is None else v[rep]) for k, v in px.items()}, **usual)
        assert torch.equal(u, want), f"num_return_sequences fan_out {fan}: not the call on the repeated inputs"
    skw = dict(prompt_lookup_num_tokens=3, speculate_selection="any", return_dict_in_generate=True)
    for kw in (usual, dict(usual, **pc.configs_from(plain, T)["all_five"][0])):
        want = _gen(model, ids, px, **kw)
        got = _gen(model, ids, px, **kw, **skw)
        assert got.speculation is not None, "the request was not served"
        assert np.array_equal(got.sequences.numpy(), want.numpy()), "speculation changes the ids of a warped sampled call"


def check_pooled_sessions(model, B=2):
    """two sessions in the decode pool at once with different warper settings: each returns its lone call's ids (the values travel in
    the rows' records, the captured step is shared)"""
    ids, px = inputs_for(B)
    args = (ids, px["images"], px["segs"], px["depths"])
    root = model.engine
    kws = [dict(do_sample=True, temperature=TEMP, top_k=0, seed=5, min_p=1.0),
           dict(do_sample=True, temperature=TEMP, top_k=0, seed=5, typical_p=1e-4),
           dict(do_sample=True, temperature=TEMP, top_k=30, top_p=0.95, seed=5, **WARP)]
    lone = [root.generate(*args, max_new_tokens=N_NEW, **kw) for kw in kws]
    assert np.array_equal(lone[0], root.generate(*args, max_new_tokens=N_NEW)) and not np.array_equal(lone[1], lone[0])
    sessions = [root, root.fork(), root.fork()]
    outs, errs = [[None] * 3 for _ in sessions], []

    def work(si):
        try:
            for j in range(3):
                outs[si][j] = sessions[si].generate(*args, max_new_tokens=N_NEW, **kws[(si + j) % 3])
        except BaseException as e:
            errs.append(e)

    try:
        ths = [threading.Thread(target=work, args=(i,)) for i in range(3)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
        for si in range(3):
            for j in range(3):
                assert np.array_equal(outs[si][j], lone[(si + j) % 3]), f"session {si} call {j}: pooled ids differ from the lone call's"
    finally:
        for s in sessions[1:]:
            s.close()


def check_no_leak_and_refusals(model, B=2):
    """nothing leaks into the next call — behind a warped call, behind one that failed, behind a request another entry point consumed
    or a greedy call ignored — and every refusal (Python and C) comes before the engine is touched and leaves it usable"""
    eng = model.engine
    ids, px = inputs_for(B)
    T = ids.shape[1]
    args = (ids, px["images"], px["segs"], px["depths"])
    greedy = _gen(model, ids, px)
    skw = dict(do_sample=True, temperature=TEMP, top_k=0, seed=5)
    free = _gen(model, ids, px, **skw)
    assert not torch.equal(free, greedy)
    assert torch.equal(_gen(model, ids, px, **skw, min_p=1.0), greedy)
    assert torch.equal(_gen(model, ids, px, **skw), free), "a sampled call behind a warped one is warped"
    try:
        _gen(model, ids, px, **skw, min_p=1.0, max_new_tokens=model.config.max_position_embeddings)
        raise AssertionError("a call over the KV capacity was accepted")
    except (ValueError, RuntimeError, IndexError):
        pass
    assert torch.equal(_gen(model, ids, px, **skw), free), "a warped call that failed left its request behind"
    req = lambda *v: eng.lib.vc_request_sampling_warpers(eng._model, *(C.c_float(x) for x in v))
    gen = lambda **kw: eng.generate(*args, max_new_tokens=N_NEW, **kw)
    ekw = dict(do_sample=True, temperature=TEMP, top_k=0, seed=5)
    assert np.array_equal(gen(**ekw), free[:, T:].numpy())
    assert req(1.0, 1.0, 0.0, 0.0) == 0
    eng.prefill(*args)
    assert np.array_equal(gen(**ekw), free[:, T:].numpy()), "a request outlived another entry point"
    assert req(1.0, 1.0, 0.0, 0.0) == 0
    assert np.array_equal(gen(), greedy[:, T:].numpy())   # a greedy call: ignored and cleared
    assert np.array_equal(gen(**ekw), free[:, T:].numpy()), "a request outlived a greedy call"
    assert req(1.0, 1.0, 0.0, 0.0) == 0
    assert np.array_equal(gen(**ekw), greedy[:, T:].numpy()), "a request through the ABI alone does nothing"
    assert np.array_equal(gen(**ekw), free[:, T:].numpy())
    # refusals of the C entry leave a pending request as it was
    assert req(1.0, 1.0, 0.0, 0.0) == 0
    for bad in ((-0.1, 1.0, 0.0, 0.0), (1.5, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, 1.0, -0.1, 0.0),
                (0.0, 1.0, 0.0, 1.0), (0.0, 1.0, 0.0, -0.5), (float("nan"), 1.0, 0.0, 0.0), (0.0, float("nan"), 0.0, 0.0)):
        assert req(*bad) == -1, f"vc_request_sampling_warpers{bad} was accepted"
    assert np.array_equal(gen(**ekw), greedy[:, T:].numpy()), "a refused request changed the pending one"
    calls = eng.step_captures()
    for kw in (dict(min_p=-0.1), dict(min_p=1.5), dict(typical_p=0.0), dict(typical_p=-1.0), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1),
               dict(eta_cutoff=1.0), dict(eta_cutoff=-0.1)):
        for extra in ({}, skw, dict(num_beams=2)):
            try:
                _gen(model, ids, px, **kw, **extra)
                raise AssertionError(f"generate({kw}, {list(extra)}) was accepted")
            except ValueError:
                pass
        try:
            gen(**ekw, **kw)
            raise AssertionError(f"HipEngine.generate({kw}) was accepted")
        except ValueError:
            pass
    assert eng.step_captures() == calls
    assert torch.equal(_gen(model, ids, px, **skw), free) and torch.equal(_gen(model, ids, px), greedy), "a refusal changed the next call"


def check_beam_sample(model, B=2):
    """beam-sample (the host loop): the warpers run behind its top-p with min_tokens_to_keep = 2 — every call of the restatement
    there returns what Transformers' classes return at 2 for its input — and change the ids of the call without them"""
    from unittest import mock

    ids, px = inputs_for(B)
    kw = dict(num_beams=2, do_sample=True, temperature=TEMP, top_k=30, top_p=0.95, seed=7, max_new_tokens=4)
    base = _gen(model, ids, px, **kw)
    seen = []
    real = lp.apply_warpers

    def spy(scores, *a, **k):
        out = real(scores, *a, **k)
        seen.append((scores.clone(), a, k, out.clone()))
        return out

    wkw = dict(min_p=0.3, typical_p=0.5, epsilon_cutoff=0.05, eta_cutoff=0.1)
    with mock.patch.object(lp, "apply_warpers", spy):
        got = _gen(model, ids, px, **kw, **wkw)
    assert len(seen) == 4, f"{len(seen)} calls of apply_warpers in 4 steps"
    for scores, a, k, out in seen:
        assert a == (0.3, 0.5, 0.05, 0.1) and k == dict(min_tokens_to_keep=2) and scores.shape[0] == 2 * B
        want = hf_chain(scores.numpy(), 1.0, 0, 1.0, *a, min_tokens_to_keep=2, head=False)
        assert torch.equal(out, want) and int(torch.isfinite(out).sum(1).min()) >= 2
    assert torch.equal(got, _gen(model, ids, px, **kw, **wkw)) and got.shape[0] == B
    assert not torch.equal(got, base) or got.shape != base.shape, "the warpers change nothing in beam-sample: the case shows nothing"
