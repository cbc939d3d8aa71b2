"""TEST INFRASTRUCTURE — generates tests/golden/score_cases.npz: what the REAL reference (imported through oracle/ref_shim.py, CPU
fp32, the seeded synthetic checkpoints of the other fixtures) makes of `labels`.

Run on the build machine only:   python tools/gen_score_golden.py

Per case the file holds the inputs (`ids`, `labels`, which pixel inputs are present), the reference's spliced labels (`new_labels`
of prepare_inputs_labels_for_multimodal), the `loss` of its own forward(labels=...) and `ref_logprobs` [B, S]: float64 log-softmax of the reference's logits
at the shifted labels (0 where nothing is scored).  Where a case runs a committed fixture's own ids, the logits are that fixture's
`prefill_logits` (checked against the live forward), so the archive does not depend on the low bits of this host's GEMMs; the one case
with edited ids takes the live logits, rounded to 1e-5.  Data only; the weights and pixels are regenerated from (variant, seed) by
vcoder_amd/synth.py.  Threads and seed are pinned as oracle/gen_golden.py pins them, member timestamps are fixed.
"""
from __future__ import annotations

import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden as gg  # noqa: E402
from vcoder_amd import config as vcfg  # noqa: E402
from vcoder_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "score_cases.npz")
IGNORE = -100

# (case, fixture whose ids / pixel choices it takes, label pattern, edit of the ids)
#   answer : the second half of the text positions labelled with their own ids
#   text   : every text position labelled with its own id
#   placeholders : `text` + token numbers written at the placeholder positions (never read by the splice)
#   none   : no label at all (loss = nan)
CASES = [
    ("ds_img_text_seg", "ds_img_text_seg", "text", None),          # DS drops the labelled text between <image> and <seg>
    ("ds_img_seg_depth", "ds_img_seg_depth", "answer", None),      # B = 2
    ("ds_zero_depth", "ds_zero_depth", "placeholders", None),      # the depth placeholder stays in the text path
    ("vc_img_text_seg", "vc_img_text_seg", "text", None),          # non-DS keeps that text
    ("llava_img", "llava_img", "answer", None),
    ("ds_unequal", "ds_img_seg_depth", "text", "drop_last_depth"),  # unequal spliced lengths, no attention mask: right pad, -100
    ("ds_no_label", "ds_img_seg", "none", None),
]


def make_labels(ids: np.ndarray, pattern: str) -> np.ndarray:
    lab = np.full_like(ids, IGNORE)
    if pattern == "none":
        return lab
    for b in range(ids.shape[0]):
        text = np.nonzero(ids[b] >= 0)[0]
        keep = text[len(text) // 2:] if pattern == "answer" else text
        lab[b, keep] = ids[b, keep]
        if pattern == "placeholders":
            ph = np.nonzero(ids[b] < 0)[0]
            lab[b, ph] = 5 + np.arange(len(ph))
    return lab


def write_npz(path: str, arrays: dict):
    """np.savez with fixed member timestamps (byte-for-byte reproducible)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


@torch.no_grad()
def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {"cases": np.array(json.dumps([c[0] for c in CASES]))}
    models = {}
    for name, fixture, pattern, edit in CASES:
        g = np.load(os.path.join(GOLD, fixture + ".npz"))
        variant, seed = str(g["variant"]), int(g["seed"])
        cfg = vcfg.tiny(variant)
        if variant not in models:
            with tempfile.TemporaryDirectory() as d:
                gg.make_clip_dir(cfg, d)
                cfg.mm_vision_tower = d
                models[variant] = gg.build_reference_model(cfg, synth.synth_state_dict(cfg, seed), d)
        model = models[variant]
        ids = g["input_ids"].copy()
        if edit == "drop_last_depth":   # the last row loses its <depth> placeholder: its spliced row is shorter
            ids[-1][ids[-1] == -400] = 7
        B = ids.shape[0]
        imgs, segs, deps = synth.synth_batch(B, cfg.vit_image_size)
        if bool(g["zero_depth"]):
            deps = np.zeros_like(deps)
        use_seg, use_depth = bool(g["use_seg"]), bool(g["use_depth"])
        labels = make_labels(ids, pattern)
        kw = {"images": torch.from_numpy(imgs)}
        pos = [torch.from_numpy(imgs)]
        if variant != "llava":
            kw["segs"] = torch.from_numpy(segs) if use_seg else None
            pos.append(kw["segs"])
        if variant == "vcoder_ds":
            kw["depths"] = torch.from_numpy(deps) if use_depth else None
            pos.append(kw["depths"])
        tid, tl = torch.from_numpy(ids), torch.from_numpy(labels)
        res = model(input_ids=tid, labels=tl, use_cache=False, **kw)
        new_labels = model.prepare_inputs_labels_for_multimodal(tid, None, None, tl, *pos)[4].numpy().astype(np.int64)
        live = res.logits.float().numpy()
        from_fixture = edit is None and "prefill_logits" in g.files
        if from_fixture:   # the same forward the fixture recorded
            assert float(np.abs(g["prefill_logits"] - live).max()) < 1e-5
        lg = torch.from_numpy(g["prefill_logits"] if from_fixture else live).double()
        S = lg.shape[1]
        assert new_labels.shape == (B, S)
        lp = torch.log_softmax(lg[:, :-1], -1)
        tgt = torch.from_numpy(new_labels[:, 1:])
        m = tgt != IGNORE
        ref_lp = np.zeros((B, S), dtype=np.float64)
        ref_lp[:, 1:] = torch.where(m, lp.gather(-1, tgt.clamp(min=0)[..., None])[..., 0], torch.zeros(())).numpy()
        loss = float(res.loss)
        n_scored = int(m.sum())
        chk = float(-ref_lp.sum() / n_scored) if n_scored else float("nan")
        print(f"[{name}] variant={variant} B={B} T={ids.shape[1]} S={S} scored={n_scored} loss={loss:.7f} (from its logits {chk:.7f})")
        assert (np.isnan(loss) and n_scored == 0) or abs(loss - chk) < 2e-5
        if not from_fixture:
            ref_lp = np.round(ref_lp, 5)
        out[name + "__fixture"] = np.array(fixture)
        out[name + "__ids"] = ids.astype(np.int64)
        out[name + "__labels"] = labels.astype(np.int64)
        out[name + "__new_labels"] = new_labels
        out[name + "__loss"] = np.float32(loss)
        out[name + "__ref_logprobs"] = ref_lp
        out[name + "__max_abs_logit"] = np.float32(round(float(lg.abs().max()), 4))
    write_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
