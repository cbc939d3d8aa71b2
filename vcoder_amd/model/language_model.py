"""The reference's model API on top of the HIP engine.

Mirrors (same names, arguments, return conventions and error behaviour):
  VCoderDSLlavaLlamaForCausalLM   vcoder_llava/model/language_model/vcoder_ds_llava_llama.py:41-142
  VCoderLlavaLlamaForCausalLM     vcoder_llava/model/language_model/vcoder_llava_llama.py:40-139
  LlavaLlamaForCausalLM           vcoder_llava/model/language_model/llava_llama.py
and the parts of HF `GenerationMixin.generate` the reference's callers use (SURVEY.md Appendix C;
callers: serve/cli.py:122-132, serve/chat.py:141-151, eval/model_seg_loader.py:129-139).
No torch.nn / HF Transformers module is involved: forward/generate marshal to libvcoder_hip.so.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np

from ..config import VCoderConfig
from .. import logits_processors as _lp
from ..constraints import TokenAutomaton
from ..engine import HipEngine
from .projector import build_depth_projector, build_seg_projector, build_vision_projector
from .vision_tower import build_vision_tower


class CausalLMOutputWithPast(dict):
    """Attribute + mapping access like transformers.modeling_outputs.CausalLMOutputWithPast."""

    def __init__(self, loss=None, logits=None, past_key_values=None, hidden_states=None, attentions=None):
        super().__init__(loss=loss, logits=logits, past_key_values=past_key_values, hidden_states=hidden_states,
                         attentions=attentions)
        self.__dict__ = self

    def __getitem__(self, k):
        if isinstance(k, int):
            return [v for v in (self.loss, self.logits, self.past_key_values) if v is not None][k]
        return dict.__getitem__(self, k)


class KVCacheHandle:
    """Opaque `past_key_values`: the cache lives in the engine (K key-major, V transposed, per layer); this handle
    only proves which prefill it belongs to.  `[-1][-1].shape[-2]` (how vcoder_ds_llava_arch.py:132 reads the past
    length) is supported."""

    def __init__(self, model, generation: int, length: int, batch: int):
        self._model, self.generation, self.length, self.batch = model, generation, length, batch

    def get_seq_length(self) -> int:
        return self.length

    def __bool__(self):
        return True

    def __getitem__(self, i):
        shape = (self.batch, self._model.config.num_attention_heads, self.length, self._model.config.head_dim)
        t = SimpleNamespace(shape=shape)
        return (t, t)

    def __len__(self):
        return self._model.config.num_hidden_layers

    def crop(self, length: int):
        """HF DynamicCache.crop: the cache steps back to `length` positions (the prompt's spliced length <= length <= the current
        length; nothing is copied).  A forward over this handle with one id or with several ids continues from there — how K
        candidate answers are scored behind one prefilled prompt."""
        if self.generation != self._model._generation:
            raise RuntimeError("past_key_values does not belong to the engine's current KV cache")
        self._model.engine.rewind(int(length))
        self.length = int(length)


class GenerateOutput(dict):
    """What generate(return_dict_in_generate=True / output_logprobs=True / top_logprobs=K) returns; attribute + mapping access,
    out[0] = sequences.  sequences: the tensor generate() returns otherwise.  token_logprobs [B, n] float32: log p(generated token);
    top_logprobs [B, n, K] float32 / top_token_ids [B, n, K] int64: the K most likely tokens of every step, ordered by (log-prob
    descending, id ascending); sequence_logprob [B]: row sums of token_logprobs.  n = generated columns.  A row's finishing token is
    scored; positions behind it hold 0.0 / 0.0 / -1.  sequences_scores [B] float32 (num_beams != 1; HF's name): the winning
    hypothesis' sum_logprobs / len ** length_penalty.  speculation (prompt_lookup_num_tokens, when the request was served): per-row
    int arrays "steps", "tokens", "drafted", "accepted" of the verify loop (not part of the integer indexing).  Fields that were not
    requested are None."""

    def __init__(self, sequences=None, token_logprobs=None, top_logprobs=None, top_token_ids=None, sequence_logprob=None,
                 sequences_scores=None, speculation=None):
        super().__init__(sequences=sequences, token_logprobs=token_logprobs, top_logprobs=top_logprobs,
                         top_token_ids=top_token_ids, sequence_logprob=sequence_logprob, sequences_scores=sequences_scores,
                         speculation=speculation)
        self.__dict__ = self

    def __getitem__(self, k):
        if isinstance(k, int):
            return [v for v in (self.sequences, self.token_logprobs, self.top_logprobs, self.top_token_ids, self.sequence_logprob,
                                self.sequences_scores) if v is not None][k]
        return dict.__getitem__(self, k)


MAX_TOP_LOGPROBS = 32


class TokenScores(dict):
    """What score() returns: token_logprobs [B, S] (log p(label) where labels != -100 and a row stands in front, 0 elsewhere), labels
    [B, S] as the splice laid them out, sequence_logprob [B] (row sums), loss (mean of -logprob over the scored entries, nan when
    there are none) and past_key_values.  With score(top_logprobs=K): top_logprobs [B, S, K] float32 and top_token_ids [B, S, K]
    int64 — the K most likely tokens at every scored position (what the model would have said instead of the label), 0.0 / -1
    elsewhere; None otherwise."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.__dict__ = self


def _labels_in_range(labels, vocab: int) -> bool:
    lab = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
    return not bool(((lab != -100) & ((lab < 0) | (lab >= vocab))).any())


def _score_outputs(engine):
    """(token_logprobs, labels, loss) of the engine's last labelled prefill / extend as torch tensors"""
    import torch

    lp = torch.from_numpy(np.ascontiguousarray(engine.last_token_logprobs))
    sl = torch.from_numpy(np.ascontiguousarray(engine.last_spliced_labels))
    scored = sl != -100
    scored[:, 0] = False   # HF's shift: nothing stands in front of position 0
    loss = -lp[scored].mean() if bool(scored.any()) else torch.tensor(float("nan"), dtype=torch.float32)
    return lp, sl, loss.to(torch.float32)


class _InnerModel:
    """What `get_model()` returns: the plugin modules of VCoder[DS]LlavaMetaModel (vcoder_ds_llava_arch.py:30-49)."""

    def __init__(self, config: VCoderConfig):
        self.config = config
        if hasattr(config, "mm_vision_tower"):
            self.vision_tower = build_vision_tower(config, delay_load=True)
            self.mm_projector = build_vision_projector(config)
        if config.variant != "llava":
            self.seg_mm_projector = build_seg_projector(config)
            if config.use_mm2_proj:
                self.mm2_projector = build_vision_projector(config)      # dead at inference (quirk 2)
        if config.variant == "vcoder_ds":
            self.depth_mm_projector = build_depth_projector(config)      # dead at inference (quirk 1)
        self.embed_tokens = SimpleNamespace(num_embeddings=config.vocab_size, embedding_dim=config.hidden_size)

    def get_vision_tower(self):
        return getattr(self, "vision_tower", None)


class _HipCausalLMBase:
    variant = "llava"
    model_type = "llava"

    def __init__(self, config: VCoderConfig, device="cuda", _lib_override=None, operands="bf16"):
        """operands (an addition of this build): "bf16" — libvcoder_hip.so, the benchmarked path; "fp16" — libvcoder_hip_f16.so, the
        same kernels with IEEE fp16 MFMA operands: the operand precision of the reference's own GPU path (builder.py:39,142)."""
        if config.variant != self.variant:
            config.variant = self.variant
        self.config = config
        self.model = _InnerModel(config)
        self._device_str = device if isinstance(device, str) else str(device)
        idx = 0
        if ":" in self._device_str:
            idx = int(self._device_str.split(":")[1])
        self.engine = HipEngine(config, device_index=idx, lib=_lib_override, operands=operands)
        tower = self.model.get_vision_tower()
        if tower is not None:
            tower._engine = self.engine          # CLIPVisionTower.forward runs on the engine's tower kernels
        self._generation = 0
        self.training = False
        self.generation_config = SimpleNamespace(pad_token_id=config.pad_token_id, eos_token_id=config.eos_token_id,
                                                 bos_token_id=config.bos_token_id)

    # ---- nn.Module-ish surface the reference's callers touch ------------------------------------------
    @property
    def device(self):
        import torch

        return torch.device(self._device_str if ":" in self._device_str else self._device_str + ":0")

    @property
    def dtype(self):
        import torch

        return torch.bfloat16

    def get_model(self):
        return self.model

    def get_vision_tower(self):
        return self.model.get_vision_tower()

    def eval(self):
        return self

    def requires_grad_(self, flag: bool = False):
        return self

    def to(self, *a, **k):
        return self

    def half(self):
        return self

    def cuda(self, *a):
        return self

    def parameters(self):
        return iter(())

    # ---- weights ----------------------------------------------------------------------------------------
    _PLUGINS = ("mm_projector", "seg_mm_projector", "depth_mm_projector", "mm2_projector")

    def _load_tensor(self, key: str, value) -> bool:
        """one checkpoint tensor: into the engine's inference layout AND — for the adapter plugins — into the module object
        get_model() hands out, so that `get_model().mm_projector` is a loaded, callable module as in the reference
        (vcoder_ds_llava_arch.py:34-49; depth_mm_projector / mm2_projector are dead in forward but still state-dict
        complete).  -> False when the engine ignores the key (dead at inference)."""
        for name in self._PLUGINS:
            pre = f"model.{name}."
            if key.startswith(pre) and hasattr(self.model, name):
                getattr(self.model, name).load_state_dict({key[len(pre):]: value}, strict=False)
        return self.engine.load_tensor(key, value)

    def load_state_dict(self, sd, strict: bool = True):
        used = dead = 0
        for k, v in sd.items():
            if self._load_tensor(k, v):
                used += 1
            else:
                dead += 1
        return SimpleNamespace(missing_keys=[], unexpected_keys=[], used=used, dead=dead)

    def finalize_weights(self):
        self.engine.finalize()
        # tensors whose checkpoint values bf16 cannot hold (an fp16 LLM / fp32 CLIP tower, the reference's own dtypes): the engine
        # kept a lo plane for each; the bf16 fast path computes with the rounded weights, 'strict' / 'split' with hi + lo
        self.inexact_tensors = self.engine.inexact_tensors()
        if self.inexact_tensors:
            import logging

            logging.getLogger("vcoder_amd").info(
                "%d checkpoint tensors are not bf16-representable: the bf16 fast path rounds them to bf16; precision modes "
                "'split' / 'strict' compute with bf16 hi + lo planes (the checkpoint's values to ~16 mantissa bits)", self.inexact_tensors)
        tower = self.get_vision_tower()
        if tower is not None:
            tower.is_loaded = True
        return self

    @classmethod
    def from_pretrained(cls, model_path: str, low_cpu_mem_usage=True, device="cuda", config=None, weight_format="bf16",
                        operands="bf16", **kwargs):
        """Loads config.json + weight shards; the CLIP tower comes from the checkpoint if present, else from the
        local directory `config.mm_vision_tower` (the reference downloads it: clip_encoder.py:22-27 — there is no
        network here, so a hub name that is not a local directory is an error)."""
        import os

        from .. import checkpoint

        if config is not None and not isinstance(config, VCoderConfig):
            # an HF PretrainedConfig handed over by AutoModelForCausalLM.from_pretrained (vcoder_amd/hf_register.py)
            config = VCoderConfig.from_hf_dict(config.to_dict(), os.path.basename(os.path.normpath(str(model_path))))
        cfg = config if config is not None else VCoderConfig.from_pretrained(model_path, os.path.basename(model_path))
        return cls.from_tensors(cfg, checkpoint.iter_checkpoint_tensors(model_path), device=device, weight_format=weight_format,
                                operands=operands)

    @classmethod
    def from_tensors(cls, cfg: VCoderConfig, tensors, device="cuda", weight_format="bf16", _lib_override=None, operands="bf16"):
        """A model from an iterator of (HF state-dict key, tensor) pairs — one checkpoint, or a base checkpoint overlaid with
        merged LoRA deltas / projector weights (model/builder.py).  The CLIP tower comes from the stream when it carries
        `vision_tower` keys, else from the local directory `config.mm_vision_tower`."""
        model = cls(cfg, device=device, _lib_override=_lib_override, operands=operands)
        saw_tower = False
        for k, v in tensors:
            saw_tower |= "vision_tower" in k
            model._load_tensor(k, v)
        if not saw_tower:
            model.get_vision_tower().load_model(engine=model.engine)
        if weight_format != "bf16":
            model.engine.set_weight_format(weight_format)   # W8A16: quantised on the device at finalize
        model.finalize_weights()
        return model

    # ---- forward (vcoder_ds_llava_llama.py:57-118) ----------------------------------------------------------
    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, inputs_embeds=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, images=None, segs=None, depths=None,
                return_dict=None):
        """labels [B, T] (aligned with input_ids, -100 = ignored): `loss` is the reference's (vcoder_ds_llava_llama.py:95-106) — the
        labels are spliced like the embeddings, shifted by one, and the mean of -log p(label) over the labelled positions comes
        back as a float32 scalar (nan when nothing is labelled), first in the tuple with return_dict=False (:108-110).  It is
        computed on the device from the labelled rows alone (HipEngine.prefill(labels=)); no gradient exists."""
        return self._forward(input_ids, attention_mask, past_key_values, labels, use_cache, output_attentions, output_hidden_states,
                             images, segs, depths, return_dict, want_logits=True)

    def score(self, input_ids, labels, images=None, segs=None, depths=None, past_key_values=None, attention_mask=None,
              top_logprobs: int = 0):
        """log p(label) per token without logits leaving the device: same dispatch as forward (prefill with images, text-only
        prefill, continuation of `past_key_values`), no all-row logits.  -> TokenScores.  Candidate answers behind one prompt:
        prefill once, then per candidate score(candidate_ids, candidate_ids, past_key_values=pkv) and pkv.crop(prompt_length).
        top_logprobs = K (0 .. 32): additionally the K most likely tokens at every scored position (TokenScores.top_logprobs /
        top_token_ids), ordered by (log-prob descending, id ascending)."""
        if labels is None:
            raise ValueError("score() needs labels")
        K = int(top_logprobs or 0)
        if K < 0 or K > MAX_TOP_LOGPROBS:
            raise ValueError(f"top_logprobs must be in 0 .. {MAX_TOP_LOGPROBS}, got {K}")
        return self._forward(input_ids, attention_mask, past_key_values, labels, None, None, None, images, segs, depths, None,
                             want_logits=False, top_logprobs=K)

    def _forward(self, input_ids, attention_mask, past_key_values, labels, use_cache, output_attentions, output_hidden_states,
                 images, segs, depths, return_dict, want_logits, top_logprobs=0):
        import torch

        if labels is not None:
            lab_shape = tuple(labels.shape) if hasattr(labels, "shape") else np.asarray(labels).shape
            if input_ids is not None and lab_shape != tuple(input_ids.shape):
                raise ValueError(f"labels must have the shape of input_ids {tuple(input_ids.shape)}, got {lab_shape}")
        # The reference OVERWRITES a caller's inputs_embeds with what prepare_inputs_labels_for_multimodal returns
        # (vcoder_ds_llava_llama.py:79: the spliced embeddings, or None) — the argument is dead; without input_ids the call
        # then dies in LlamaModel ("You must specify exactly one of input_ids or inputs_embeds").  Same here.
        if input_ids is None:
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds (the reference discards a caller's "
                             "inputs_embeds: vcoder_ds_llava_llama.py:79)")
        ids = input_ids
        B = ids.shape[0]
        if past_key_values is not None and ids.shape[1] == 1:
            # cached decode step: the input_ids.shape[1]==1 fast path (vcoder_ds_llava_arch.py:130-133)
            if not isinstance(past_key_values, KVCacheHandle) or past_key_values.generation != self._generation:
                raise RuntimeError("past_key_values does not belong to the engine's current KV cache")
            tok = ids.reshape(-1).detach().cpu().numpy() if hasattr(ids, "detach") else np.asarray(ids).reshape(-1)
            # With images the reference REPLACES the mask by ones here (vcoder_ds_llava_arch.py:130-133): keys a padded
            # prefill hid become visible.  Without images the caller's mask goes through to LlamaModel: the engine keeps the
            # prefill's hidden keys hidden (new positions are visible, as HF's generate loop appends ones).
            if images is not None or attention_mask is None:
                self.engine.clear_attention_mask()
            # output_hidden_states / output_attentions of a cached step: [B, 1, D] per entry, [B, H, 1, past + 1] per layer
            if labels is not None:   # before the step: a refused call leaves the cache as it was
                lab1 = np.asarray(labels.detach().cpu().numpy() if hasattr(labels, "detach") else labels, dtype=np.int64)
                if lab1.shape != (B, 1):
                    raise ValueError(f"labels must be [{B},1], got {tuple(lab1.shape)}")
                if not _labels_in_range(lab1, self.config.vocab_size):
                    raise IndexError("Target is out of bounds.")
            lg, _ = self.engine.decode_step(tok, hidden_states=bool(output_hidden_states), attentions=bool(output_attentions))
            past_key_values.length += 1
            logits = torch.from_numpy(lg).unsqueeze(1)
            pkv = past_key_values
            if labels is not None:   # one new position: the shift leaves nothing to score (torch's mean over an empty set)
                self.engine.last_token_logprobs = np.zeros((B, 1), dtype=np.float32)
                self.engine.last_spliced_labels = lab1
                self.engine.last_top_logprobs = np.zeros((B, 1, top_logprobs), dtype=np.float32) if top_logprobs else None
                self.engine.last_top_ids = np.full((B, 1, top_logprobs), -1, dtype=np.int32) if top_logprobs else None
        elif past_key_values is not None:
            # multi-token continuation of the cache: with images=None, prepare_inputs_labels_for_multimodal returns early
            # (vcoder_ds_llava_arch.py:129-133) and LlamaModel runs the n new ids at positions past .. past+n-1, causal inside
            # the chunk, over every cached key.  Every check comes before the engine is touched: a refused call leaves the
            # cache, its mask and the live handles as they were.
            if images is not None:
                raise NotImplementedError("continuing a cached sequence with several new ids AND images is not supported: the "
                                          "image features would have to be spliced into the continuation")
            if not isinstance(past_key_values, KVCacheHandle) or past_key_values.generation != self._generation:
                raise RuntimeError("past_key_values does not belong to the engine's current KV cache")
            tok = ids.detach().cpu().numpy() if hasattr(ids, "detach") else np.asarray(ids)
            n = tok.shape[1]
            if B != past_key_values.batch:
                raise ValueError(f"input_ids has {B} rows, past_key_values {past_key_values.batch}")
            if ((tok < 0) | (tok >= self.config.vocab_size)).any():
                raise IndexError("index out of range in self")
            if labels is not None and not _labels_in_range(labels, self.config.vocab_size):
                raise IndexError("Target is out of bounds.")   # torch's CrossEntropyLoss
            if past_key_values.length + n > self.config.max_position_embeddings // 64 * 64:   # vc_extend's own limit
                raise RuntimeError(f"KV cache full: position {past_key_values.length + n} exceeds max_position_embeddings="
                                   f"{self.config.max_position_embeddings}")
            if attention_mask is not None:
                am = attention_mask.detach().cpu().numpy() if hasattr(attention_mask, "detach") else np.asarray(attention_mask)
                if am.ndim != 2 or am.shape[0] != B or am.shape[1] < n:
                    raise ValueError(f"attention_mask must be [{B}, past + {n}], got {tuple(am.shape)}")
                # the rule of the 1-token path: the prefill's hidden keys stay hidden, the new positions are visible
                if not bool(np.all(am[:, -n:] != 0)):
                    raise NotImplementedError("an attention_mask that hides some of the NEW positions of a cached continuation "
                                              "is outside the VCoder hot path")
            else:
                self.engine.clear_attention_mask()
            _, full = self.engine.extend(tok, all_logits=want_logits, hidden_states=bool(output_hidden_states),
                                         attentions=bool(output_attentions), labels=labels, top_logprobs=top_logprobs)
            past_key_values.length += n
            logits = torch.from_numpy(full) if want_logits else None
            pkv = past_key_values
        else:
            # images None: prepare_inputs_labels_for_multimodal returns early (vcoder_ds_llava_arch.py:129-133) and the
            # call is a plain Llama forward over the text ids
            if images is None and attention_mask is not None and not _all_ones(attention_mask):
                # (before the prefill: a refused call must leave the engine's cache and the live KVCacheHandles as they were)
                raise NotImplementedError("a padded TEXT-ONLY batch (attention_mask with zeros, images=None) is outside the "
                                          "VCoder hot path")
            _, full, S = self.engine.prefill(ids, images, (segs if self.variant != "llava" else None) if images is not None else None,
                                             (depths if self.variant == "vcoder_ds" else None) if images is not None else None,
                                             all_logits=want_logits, reserve=self._decode_reserve,
                                             attention_mask=attention_mask if images is not None else None,
                                             hidden_states=bool(output_hidden_states), attentions=bool(output_attentions),
                                             labels=labels, top_logprobs=top_logprobs)
            self._generation += 1
            logits = torch.from_numpy(full) if want_logits else None
            pkv = KVCacheHandle(self, self._generation, S, B)
        loss = None
        if labels is not None:
            lp, sl, loss = _score_outputs(self.engine)
            if not want_logits:
                tlp = tid = None
                if top_logprobs:
                    tlp = torch.from_numpy(np.ascontiguousarray(self.engine.last_top_logprobs))
                    tid = torch.from_numpy(np.ascontiguousarray(self.engine.last_top_ids).astype(np.int64))
                return TokenScores(token_logprobs=lp, labels=sl, sequence_logprob=lp.sum(dim=1), loss=loss, past_key_values=pkv,
                                   top_logprobs=tlp, top_token_ids=tid)
        if hasattr(ids, "device") and getattr(ids, "is_cuda", False):
            logits = logits.to(ids.device)
        hs = None
        if output_hidden_states and self.engine.last_hidden_states is not None:
            # the tuple LlamaModel.forward returns: inputs_embeds, every layer's output, the last one after the final norm
            hs = tuple(torch.from_numpy(h) for h in self.engine.last_hidden_states)
        at = None
        if output_attentions and self.engine.last_attentions is not None:
            at = tuple(torch.from_numpy(a) for a in self.engine.last_attentions)     # L tensors [B, H, S, S]
        out = CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=pkv if use_cache is not False else None,
                                     hidden_states=hs, attentions=at)
        if return_dict is False:
            return ((loss,) if loss is not None else ()) + (out.logits,) + \
                ((out.past_key_values,) if out.past_key_values is not None else ())
        return out

    __call__ = forward

    # KV slots a forward() prefill keeps free for the caller's cached decode steps (an HF-style external generate loop
    # drives forward once per token); the cache grows if the loop runs longer
    _decode_reserve = 512

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, attention_mask=None, inputs_embeds=None,
                                      **kwargs):
        """vcoder_ds_llava_llama.py:120-142"""
        if past_key_values:
            input_ids = input_ids[:, -1:]
        model_inputs = {"inputs_embeds": inputs_embeds} if (inputs_embeds is not None and past_key_values is None) \
            else {"input_ids": input_ids}
        model_inputs.update({"past_key_values": past_key_values, "use_cache": kwargs.get("use_cache"),
                             "attention_mask": attention_mask, "images": kwargs.get("images", None)})
        if self.variant != "llava":
            model_inputs["segs"] = kwargs.get("segs", None)
        if self.variant == "vcoder_ds":
            model_inputs["depths"] = kwargs.get("depths", None)
        return model_inputs

    # ---- generate (HF GenerationMixin subset) ---------------------------------------
    def generate(self, input_ids=None, inputs=None, images=None, segs=None, depths=None, do_sample: bool = False,
                 temperature: float = 1.0, top_p: Optional[float] = None, top_k: Optional[int] = None, num_beams: int = 1,
                 max_new_tokens: Optional[int] = None, max_length: Optional[int] = None, streamer=None,
                 use_cache: bool = True, stopping_criteria=None, eos_token_id=None, pad_token_id=None,
                 attention_mask=None, generator=None, seed: Optional[int] = None, return_dict_in_generate: bool = False,
                 output_logprobs: bool = False, top_logprobs: int = 0, repetition_penalty: Optional[float] = None,
                 no_repeat_ngram_size: Optional[int] = None, min_new_tokens: Optional[int] = None, min_length: Optional[int] = None,
                 bad_words_ids=None, processors_on_device: bool = True, prompt_lookup_num_tokens: Optional[int] = None,
                 max_matching_ngram_size: int = 2, lookup_ids=None, num_return_sequences: int = 1, fan_out: bool = False,
                 speculate_selection: str = "greedy", constraint=None, prefix_allowed_tokens_fn=None,
                 guidance_scale: Optional[float] = None, negative_prompt_ids=None, negative_prompt_attention_mask=None,
                 negative_images=None, negative_segs=None, negative_depths=None, min_p: Optional[float] = None,
                 typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None,
                 **kwargs):
        """Returns cat(input_ids, new_ids) [B, T+n] int64 — the prompt part keeps its negative placeholder ids,
        callers slice `[:, T:]` (serve/cli.py:135).

        return_dict_in_generate / output_logprobs / top_logprobs = K (0 .. 32; implies output_logprobs): a GenerateOutput instead —
        `sequences` (that tensor), `token_logprobs` [B, n], `top_logprobs` / `top_token_ids` [B, n, K], `sequence_logprob` [B]; what
        was not asked for is None.  The log-probs are those of the model's own next-token distribution: log_softmax of the step's
        fp32 logits, taken BEFORE temperature / top-k / top-p — also when sampling (the probability the model gave the token, not
        the one the warped distribution drew it with).  For greedy decoding this is what HF's
        compute_transition_scores(..., normalize_logits=True) gives.  Ties order by the lower id, as the greedy argmax.  A row's
        finishing token (EOS / the token completing a stop sequence) is scored; later positions hold 0.0 / 0.0 / -1.  They come from
        a kernel behind every selection of the device loop (the call then runs on the session's own loop, not in the decode pool);
        the host fallback loop computes the same from its logits.  HF's full-vocabulary `output_scores` is not implemented: with
        return_dict_in_generate it raises, alone it is ignored as before.

        repetition_penalty (1.0) / no_repeat_ngram_size (0) / bad_words_ids (None) / min_length (0) / min_new_tokens (0): HF's logits
        processors, in 4.31's order, over the history input_ids + generated ids — RepetitionPenaltyLogitsProcessor
        (score < 0 ? score * p : score / p), NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor (sequences that are one EOS id
        are dropped), MinLengthLogitsProcessor (counts the un-spliced input_ids, like HF) and MinNewTokensLengthLogitsProcessor (every
        EOS id is -inf; stop sequences are unaffected).  History ids outside the vocabulary — the negative image placeholders — are
        skipped; HF itself would raise an index error on them in the repetition penalty.  With the defaults nothing changes (the
        call takes the path it took, decode pool included).  Otherwise a kernel in front of every selection of the device loop
        applies them (greedy and sampled calls; the call runs on the session's own loop); more than 32 bad words, one longer than 8
        ids, more than 9 EOS ids or processors_on_device=False take the host loop, which applies the same processors in torch in
        front of the warpers and returns the same ids.  Beam search with a processor set runs on the host loop, which applies them to
        log_softmax(logits) before the beam scores are added, as 4.31's beam_search.  Log-probs (output_logprobs / top_logprobs)
        stay those of the model's own distribution: the raw logits, before processors as well as before warpers.  Invalid values
        raise ValueError before the engine is touched.

        constraint (a constraints.TokenAutomaton) / prefix_allowed_tokens_fn (HF's callable fn(batch_id, input_ids) -> allowed ids):
        constrained decoding with HF 4.31's PrefixConstrainedLogitsProcessor semantics — behind the processors above, in front of
        the warpers, the ids the callable does not return are -inf (an empty list: the whole row).  A callable cannot run inside a
        captured step, so prefix_allowed_tokens_fn always takes the host loops.  `constraint` states the same restriction as a
        deterministic automaton over token ids ("one of these strings": TokenAutomaton.from_sequences; "a separated list drawn
        from these classes": from_list; raw tables: from_edges) whose state the device loop keeps per row: a fourth phase of the
        processor kernel masks the processed row in front of every selection — greedy and sampled calls, every precision mode,
        with or without the processors, with log-probs (still those of the raw rows), EOS ids, stop sequences, a streamer and
        num_return_sequences in both forms; the call runs on the session's own loop.  Its definition is
        constraint.as_prefix_allowed_tokens_fn(T): whatever takes the host loop — processors_on_device=False, a stopping criterion
        that needs host code, num_beams > 1 (`_beam_search`, which applies it to log_softmax(logits) before the beam scores are
        added) — runs under that callable and returns the same tensor.  The automaton starts at the first generated token; rows
        that are finished are not constrained (they emit pad).  prompt_lookup_num_tokens is not served beside a constraint (the
        call runs as without it, `speculation` is None).  Both arguments together, or a wrong type, raise ValueError before the
        engine is touched; without either every call takes the path it took.

        num_beams = n > 1: beam search (HF 4.31's beam_search + BeamSearchScorer; `length_penalty`, `early_stopping` as keyword
        arguments).  Without sampling and stopping criteria, outside strict mode and with B * n <= 16 rows it runs inside the device
        loop too (vc_generate_beam: one captured beam step per token, fp32 scores, ties by the lower flat index beam * V + id);
        beam-sample, stopping criteria and strict mode — or beam_on_device=False — take the host loop `_beam_search`.  Both return
        the same tensor; with return_dict_in_generate the GenerateOutput carries `sequences_scores` [B].

        prompt_lookup_num_tokens = k (1 .. 7; current Transformers' name), max_matching_ngram_size (1 .. 4, default 2), lookup_ids:
        prompt-lookup speculative decoding inside the device loop.  Every step drafts up to k ids — those behind the latest earlier
        occurrence of the sequence's last n-gram in lookup_ids + input_ids + generated ids — and verifies them as k + 1 rows of ONE
        weight pass; as long as the drafts are what the model itself picks they are emitted together.  The returned ids,
        their number and the log-probs are exactly (array_equal) those of the call without the argument; only the step count
        drops.  lookup_ids (a list of B id lists; one list for B = 1) is what the caller expects the answer to resemble: the
        previous turn, a class list.  A GenerateOutput carries `speculation` (per-row "steps", "tokens", "drafted", "accepted").
        The request is NOT served — the call runs as without it, `speculation` is None — with: sampling; a logits-processor set;
        num_beams > 1; precision "split" / "strict"; a stopping criterion that needs the host loop; B * (k + 1) > 32; a KV
        capacity whose k + 1 score rows exceed a CU's LDS.  A speculated call runs on the session's own loop, not in the decode
        pool, and closes it: decode_step / extend behind it refuse until the next prefill.  k or the n-gram size outside their
        range raise ValueError before the engine is touched.

        speculate_selection = "greedy" (the default) | "any": the selections prompt_lookup_num_tokens is served for.  "greedy" is the
        scope above, bit for bit: a sampled call, or one with a processor set, runs as without the argument.  "any" also serves
        sampled calls (temperature / top-k / top-p, any seed) and calls with a device-resident processor set (greedy or sampled),
        with log-probs, EOS ids, stop sequences, a streamer, and num_return_sequences = n in its default (repeated-prompt) form while
        B n (k + 1) <= 32.  The device sampler is a Gumbel-max keyed by (seed, generated index, vocabulary id), so the token a row
        emits at index t is a pure function of that step's logits row, the row's parameters and t: the verify step samples query row
        j with the key of index t + j, processes it over the history plus the j drafts in front of it, and accepts a draft while it
        equals the token selected in front of it.  No acceptance probability is involved: `sequences`, their number, the log-probs
        and the streamer's pieces are exactly (array_equal) those of the same call with the same `seed` without
        prompt_lookup_num_tokens.  It is opt-in because a served call leaves the decode pool and closes the session's loop (above),
        which a sampled caller has to ask for.  Still NOT served under "any" (the call runs as without the argument, `speculation` is
        None): num_beams > 1; precision "split" / "strict"; a stopping criterion that needs the host loop;
        processors_on_device=False or a processor set that does not fit the device; fan_out=True; B (k + 1) > 32; the LDS bound of
        the verify attention.  Any other value raises ValueError before the engine is touched.

        num_return_sequences = n (HF 4.31's semantics): with do_sample=True `sequences` is [B n, T + L], rows b n + j, each carrying
        its prompt's input_ids; every GenerateOutput field is B n rows wide and the streamer receives B n-wide columns.  The result
        is exactly (array_equal) that of the call on input_ids.repeat_interleave(n, 0) with the images repeated and the same seed.
        By default the engine repeats the prompts itself.  fan_out=True: the B prompts are encoded and prefilled ONCE and each
        decode step reads a prompt's keys and values once for its n rows (the fan-out attention; engine.last_fanout["shared"]);
        that form is served for 2 <= n <= 8 in the bf16 precision mode, runs on the session's own loop and closes it (decode_step /
        extend refuse until the next prefill); otherwise — precision "split" / "strict", n > 8 — the prompts are repeated as by
        default.  It is not the default because at 7b it is faster only for B = 2, n = 8 of the shapes measured
        (profiles/fanout_wall_times.md); at 7b dims it is served only under engine.set_batch_invariant(True), the mode in which one
        prefill has the bits of each repeated copy.  The host loop (a stopping criterion that needs host code, processors_on_device=False)
        expands its inputs n times as `_beam_search` does.  n > 1 without sampling and
        num_beams == 1 raises HF's ValueError; with num_beams > 1 NotImplementedError (returning the n best beams is the beam
        scorer's business); B n above 16 ValueError.  n == 1 (the default) is the call it always was.

        guidance_scale = g, negative_prompt_ids [B, Tn] or [1, Tn] (rectangular, unpadded), negative_prompt_attention_mask,
        negative_images / negative_segs / negative_depths: classifier-free guidance with the semantics of Transformers'
        UnbatchedClassifierFreeGuidanceLogitsProcessor, the FIRST processor of the list.  Every step scores the next token behind the
        prompt (raw row c) and behind the negative prompt (raw row u), both followed by the ids generated so far, and everything
        behind it — the five processors (the repetition penalty's sign test then runs on log-domain values, as in HF), the
        constraint, the warpers, the greedy or sampled selection — reads g * (log_softmax(c) - log_softmax(u)) + log_softmax(u) in
        place of c.  Log-probs stay those of the raw conditional row; EOS, stop sequences and max_new_tokens are decided on the
        conditional stream; the processors' history is input_ids + generated ids.  Without negative_prompt_ids the negative prompt
        is HF's default, the last prompt token alone.  Placeholders in it are spliced from the negative_* pixels ([B, 3, S, S]);
        mm_utils.strip_placeholders(input_ids) — the question without its pictures — is the visual-contrastive recipe against
        object hallucination.  HF runs a second forward per token; here the unconditional row rides in the same weight pass: the
        device loop steps 2 B rows (guidance_combine_kernel in front of the processor launch, guidance_follow_kernel behind the
        selection), on the session's own loop, which it closes (decode_step / extend refuse until the next prefill);
        engine.last_guidance reports it.  Served on the device with greedy and sampled selection, the processors, `constraint`,
        log-probs, EOS ids, stop sequences, a streamer and num_return_sequences (the inputs are repeated; fan_out=True falls back to
        that); processors_on_device=False, a stopping criterion that needs host code, prefix_allowed_tokens_fn and the precision
        modes "split" / "strict" take the host
        loop, which applies logits_processors.apply_guidance in front of the other processors to the 2 B rows of
        engine.prefill_guided / decode_step and returns the same ids.  prompt_lookup_num_tokens is not served beside it (the call
        runs as without it, `speculation` is None).  guidance_scale None or 1.0 is no request (HF's rule): the call takes exactly
        the path it takes without the arguments, decode pool included.  Refused before the engine is touched: a non-finite scale,
        placeholders without their pixels, a negative batch other than B or 1, zeros in the mask of a negative prompt
        (NotImplementedError for a text-only one, as a padded text-only batch), 2 B n above 16 rows (ValueError); num_beams > 1
        (NotImplementedError).

        min_p / typical_p / epsilon_cutoff / eta_cutoff: Transformers' MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and
        EtaLogitsWarper with min_tokens_to_keep = 1, behind top-p and in that order — temperature -> top-k -> top-p -> min-p ->
        typical -> epsilon -> eta -> draw — each over the survivors of those in front of it (its softmax and entropy see -inf where
        something was removed).  min_p removes p < min_p * max p; typical_p keeps, in ascending order of |-log p - H|, the tokens
        up to the one whose cumulative probability reaches it; epsilon_cutoff removes p < epsilon; eta_cutoff removes
        p < min(eta, sqrt(eta) exp(-H)); the two cutoffs spare every score that equals the maximum.  Off (HF's GenerationConfig
        rules): min_p None or 0, typical_p None or >= 1, a cutoff None or 0 — the call then takes exactly the path and returns
        exactly the ids it does without the arguments.  On the device they are four more thresholds of the sampler (warp_thresholds
        in csrc/select.hip), carried in the row's record: a call keeps the loop it would run on, the decode pool included, and
        they combine with the processors, `constraint`, guidance, log-probs (of the raw rows), num_return_sequences and
        prompt_lookup_num_tokens under speculate_selection="any".  The host sampling loop applies
        logits_processors.apply_warpers behind its top-p, beam-sample with min_tokens_to_keep = 2 (4.31's rule for beams).  Not
        applied to a greedy call, as in HF; validated all the same, before the engine is touched: ValueError for min_p outside
        [0, 1], typical_p <= 0, a cutoff outside [0, 1).

        Everything the reference's callers ask for runs on the device inside the hipGraph-replayed decode loop
        (vc_generate): greedy argmax; sampling with HF's warper order temperature -> top-k -> top-p -> multinomial
        (`top_k` defaults to 50 when sampling, HF's GenerationConfig default, which is what serve/cli.py:122-132 gets);
        EOS / pad bookkeeping; stopping criteria that reduce to token-id suffixes (KeywordsStoppingCriteria(["</s>"]));
        the streamer, fed from a callback every `stream_every` tokens.  Only a stopping criterion that needs host code
        (a text match over several tokens) falls back to the per-token decode_step loop, like the reference's HF loop.
        Sampling draws from a counter-based generator: pass `seed` (or a torch `generator`, whose initial seed is used)
        for reproducible output; bit-equality with torch.multinomial's stream is not defined."""
        import torch

        if input_ids is None:
            input_ids = inputs
        if temperature is not None and float(temperature) <= 0.0:
            do_sample = False
        # every refusal of the log-prob arguments comes before the engine is touched
        K = int(top_logprobs or 0)
        if K < 0 or K > MAX_TOP_LOGPROBS:
            raise ValueError(f"top_logprobs must be in 0 .. {MAX_TOP_LOGPROBS}, got {K}")
        want_lp = bool(output_logprobs) or K > 0
        as_dict = bool(return_dict_in_generate) or want_lp
        if return_dict_in_generate and kwargs.get("output_scores"):
            raise NotImplementedError("output_scores (HF's full-vocabulary score tuples) is not implemented: ask for "
                                      "output_logprobs=True / top_logprobs=K instead")
        if num_beams != 1 and want_lp:
            raise NotImplementedError("per-token log-probs (output_logprobs / top_logprobs) are not implemented for num_beams != 1")
        if prompt_lookup_num_tokens is not None:
            if not 1 <= int(prompt_lookup_num_tokens) <= 7:
                raise ValueError(f"prompt_lookup_num_tokens must be in 1 .. 7, got {prompt_lookup_num_tokens!r}")
            if not 1 <= int(max_matching_ngram_size) <= 4:
                raise ValueError(f"max_matching_ngram_size must be in 1 .. 4, got {max_matching_ngram_size!r}")
        if speculate_selection not in ("greedy", "any"):
            raise ValueError(f"speculate_selection must be 'greedy' or 'any', got {speculate_selection!r}")
        if constraint is not None and prefix_allowed_tokens_fn is not None:
            raise ValueError("`constraint` and `prefix_allowed_tokens_fn` state the same thing: pass one of them")
        if constraint is not None and not isinstance(constraint, TokenAutomaton):
            raise ValueError(f"`constraint` has to be a vcoder_amd.constraints.TokenAutomaton, but is {type(constraint).__name__}")
        if prefix_allowed_tokens_fn is not None and not callable(prefix_allowed_tokens_fn):
            raise ValueError(f"`prefix_allowed_tokens_fn` has to be callable, but is {type(prefix_allowed_tokens_fn).__name__}")
        warp = _lp.check_warpers(min_p, typical_p, epsilon_cutoff, eta_cutoff)   # (0.0: off)
        nrs = int(num_return_sequences)
        if nrs < 1:
            raise ValueError(f"`num_return_sequences` has to be at least 1, got {num_return_sequences!r}")
        # guidance: every refusal before the engine is touched; None / 1.0 is no request and nothing below changes
        gscale = _lp.check_guidance_scale(guidance_scale)
        neg_ids = None
        if gscale is not None:
            if num_beams != 1:
                raise NotImplementedError("guidance_scale is not implemented for num_beams > 1")
            neg_ids = self._negative_prompt(input_ids, negative_prompt_ids, negative_prompt_attention_mask, negative_images,
                                            negative_segs, negative_depths)
            if 2 * input_ids.shape[0] * nrs > self.engine.MAX_BATCH:
                raise ValueError(f"a guided batch of {input_ids.shape[0]} x num_return_sequences {nrs} needs "
                                 f"{2 * input_ids.shape[0] * nrs} rows: a replica decodes at most {self.engine.MAX_BATCH} at a time")
        if nrs > 1:
            if num_beams != 1:
                raise NotImplementedError("num_return_sequences > 1 is not implemented for num_beams > 1: returning the n best beams "
                                          "is the beam scorer's business")
            if not do_sample:
                raise ValueError(f"`num_return_sequences` has to be 1, but is {nrs} when doing greedy search.")   # HF's own
            if input_ids.shape[0] * nrs > self.engine.MAX_BATCH:
                raise ValueError(f"batch {input_ids.shape[0]} x num_return_sequences {nrs} exceeds the {self.engine.MAX_BATCH} rows a "
                                 "replica decodes at a time")
        self.engine.last_speculation = None
        self.engine.last_fanout = None
        self.engine.last_guidance = None
        eos_all = self.config.eos_token_id if eos_token_id is None else eos_token_id
        eos_all = [int(e) for e in (eos_all if isinstance(eos_all, (list, tuple)) else ([] if eos_all is None else [eos_all]))]
        proc = _lp.make(repetition_penalty, no_repeat_ngram_size, min_new_tokens, min_length, bad_words_ids, eos_all)
        if not proc.active:
            proc = None
        if num_beams != 1:
            if streamer is not None:
                raise ValueError("`streamer` cannot be used with beam search")   # HF's own check
            sample = None
            if do_sample:   # beam-sample (the eval loaders forward --temperature and --num_beams independently)
                if generator is None:
                    generator = torch.Generator().manual_seed(int(seed if seed is not None else torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF)
                sample = dict(temperature=float(temperature or 1.0), top_k=50 if top_k is None else int(top_k),
                              top_p=1.0 if top_p is None else float(top_p), generator=generator, warp=warp)
            beam_args = (input_ids, images, segs, depths, int(num_beams), max_new_tokens, max_length, eos_token_id, pad_token_id,
                         attention_mask)
            beam_kw = (float(kwargs.get("length_penalty", 1.0)), kwargs.get("early_stopping", False),
                       kwargs.get("_beam_len_counts_prompt", True))
            # plain beam search (what the reference's eval loaders ask for) runs inside the device loop; beam-sample, stopping
            # criteria, strict mode and more rows than a replica decodes keep the host loop
            # (logits processors too: the device beam loop does not carry them)
            allowed_fn = prefix_allowed_tokens_fn
            if constraint is not None:
                allowed_fn = constraint.as_prefix_allowed_tokens_fn(input_ids.shape[1], self.config.vocab_size)
            on_device = (kwargs.get("beam_on_device", True) and sample is None and not stopping_criteria and proc is None
                         and allowed_fn is None and self.engine.precision != "strict" and input_ids.shape[0] * int(num_beams) <= self.engine.MAX_BATCH)
            if on_device:
                seqs, scores = self._beam_search_device(*beam_args, *beam_kw)
            else:
                seqs, scores = self._beam_search(*beam_args, stopping_criteria, *beam_kw, sample, return_scores=True, processors=proc,
                                                 allowed_fn=allowed_fn)
            return GenerateOutput(sequences=seqs, sequences_scores=scores) if as_dict else seqs
        T = input_ids.shape[1]
        B = input_ids.shape[0]
        if max_new_tokens is None:
            max_new_tokens = (max_length - T) if max_length is not None else 20
        eos = self.config.eos_token_id if eos_token_id is None else eos_token_id
        # HF's GenerationConfig takes one EOS id or a list: any of them finishes a row.  The first is the device loop's EOS, the
        # others end a row the same way as single-token stop sequences (token kept, pads afterwards)
        eos_more = []
        if isinstance(eos, (list, tuple)):
            eos_more = [int(e) for e in eos[1:]]
            eos = int(eos[0]) if len(eos) else None
        pad = pad_token_id if pad_token_id is not None else (self.config.pad_token_id if self.config.pad_token_id is not None else eos)
        segs = segs if self.variant != "llava" else None
        depths = depths if self.variant == "vcoder_ds" else None
        ids_cpu = input_ids.detach().cpu() if hasattr(input_ids, "detach") else torch.as_tensor(np.asarray(input_ids))
        if do_sample:
            top_k = 50 if top_k is None else int(top_k)
            top_p = 1.0 if top_p is None else float(top_p)
            if seed is None:
                seed = int(generator.initial_seed()) if generator is not None else int(torch.initial_seed())
                seed = (seed + 0x9E3779B97F4A7C15 * self._sample_calls) & 0xFFFFFFFFFFFFFFFF   # successive calls differ
                self._sample_calls += 1
        # stopping criteria that reduce to a token-id suffix match run on the device: the
        # reference's KeywordsStoppingCriteria(["</s>"]) of cli.py / the eval loaders is of that kind
        stops = []
        for crit in (stopping_criteria or []):
            seqs = crit.device_stop_sequences() if hasattr(crit, "device_stop_sequences") else _reference_keyword_stop(crit)
            if seqs is None:
                stops = None
                break
            stops += seqs
        if stops is not None:
            stops = stops + [[e] for e in eos_more]
        on_device = stops is not None and len(stops) <= 8
        if proc is not None:   # what the device kernel does not hold, or the caller's wish: the host loop applies them
            on_device = on_device and bool(processors_on_device) and proc.fits_device() and len(eos_more) <= _lp.MAX_EOS_EXTRA
        if gscale is not None:   # the caller's wish holds for a guided call as well: the host loop over engine.prefill_guided;
            # the device form is the bf16 step's: "split" / "strict" take the host loop too
            on_device = on_device and bool(processors_on_device) and self.engine.precision == "bf16"
        # a callable runs on the host; an automaton where the call is device-served anyway, else as its own callable
        if prefix_allowed_tokens_fn is not None:
            on_device = False
        if constraint is not None:
            on_device = on_device and bool(processors_on_device) and len(eos_more) <= _lp.MAX_EOS_EXTRA
        allowed_fn = prefix_allowed_tokens_fn
        if constraint is not None and not on_device:
            allowed_fn = constraint.as_prefix_allowed_tokens_fn(T, self.config.vocab_size)
        if nrs > 1:
            rep = np.repeat(np.arange(B), nrs)   # rows b n + j, as HF's _expand_inputs_for_generation

            def expand(a):
                if a is None:
                    return None
                if isinstance(a, (list, tuple)):
                    return [a[i] for i in rep]
                return a[torch.as_tensor(rep, device=a.device)] if hasattr(a, "detach") else np.asarray(a)[rep]

            prompts = ids_cpu
            ids_cpu = ids_cpu[torch.as_tensor(rep)]   # what the returned rows carry in front
            if gscale is not None:   # a guided call repeats its inputs here, both prompts: the engine sees B n sequences
                neg_ids = neg_ids[rep]
                negative_images, negative_segs, negative_depths = expand(negative_images), expand(negative_segs), expand(negative_depths)
            if not on_device or gscale is not None:   # the host loop runs over the expanded batch
                images, segs, depths, attention_mask = expand(images), expand(segs), expand(depths), expand(attention_mask)
                if lookup_ids is not None and not (B == 1 and all(np.ndim(q) == 0 for q in lookup_ids)):
                    lookup_ids = expand(list(lookup_ids))
                B = B * nrs
                prompts = ids_cpu
        else:
            prompts = ids_cpu
        gd = None
        if gscale is not None:
            neg_px = negative_images is not None
            gd = _lp.Guidance(gscale, neg_ids, negative_images, (negative_segs if self.variant != "llava" else None) if neg_px else None,
                              (negative_depths if self.variant == "vcoder_ds" else None) if neg_px else None)
            prompt_lookup_num_tokens = None   # not served beside guidance
        if streamer is not None:
            streamer.put(ids_cpu)
        if on_device:
            on_tokens = None
            if streamer is not None:
                def on_tokens(first, new_ids):   # HF feeds the streamer one [B] tensor per step
                    for j in range(new_ids.shape[1]):
                        streamer.put(torch.from_numpy(new_ids[:, j].astype(np.int64)))
            new = self.engine.generate(prompts.numpy(), images, segs, depths, max_new_tokens=max_new_tokens,
                                       eos_token_id=eos, pad_token_id=pad, stop_sequences=stops or None,
                                       do_sample=bool(do_sample), temperature=float(temperature or 1.0),
                                       top_k=top_k or 0, top_p=1.0 if top_p is None else top_p, seed=seed or 0,
                                       on_tokens=on_tokens, stream_every=kwargs.get("stream_every", 1),
                                       attention_mask=attention_mask, logprobs=want_lp, top_logprobs=K, processors=proc,
                                       eos_extra=eos_more if proc is not None else (),
                                       speculate=None if prompt_lookup_num_tokens is None else int(prompt_lookup_num_tokens),
                                       lookup_ngram=int(max_matching_ngram_size), lookup_ids=lookup_ids,
                                       speculate_selection=speculate_selection, constraint=constraint,
                                       **(dict(guidance=gd) if gd is not None else {}),
                                       **(dict(min_p=warp[0], typical_p=warp[1] or None, epsilon_cutoff=warp[2], eta_cutoff=warp[3])
                                          if do_sample and any(warp) else {}),
                                       **(dict(num_return_sequences=nrs, fan_out=bool(fan_out)) if nrs > 1 and gd is None else {}))
            self._generation += 1
            out = torch.cat([ids_cpu, torch.from_numpy(new.astype(np.int64))], dim=1)
            if want_lp:
                tok_lp, top_lp, top_id = (torch.from_numpy(np.ascontiguousarray(a)) for a in self.engine.last_generate_logprobs)
                top_id = top_id.to(torch.int64)
            if streamer is not None:
                streamer.end()
        else:
            if gd is not None:   # 2 B rows: the prompts', then the negative prompts'; a pair continues with the same token
                last, S = self.engine.prefill_guided(ids_cpu.numpy(), images, segs, depths, guidance=gd, reserve=max_new_tokens,
                                                     attention_mask=attention_mask)
            else:
                last, _, S = self.engine.prefill(ids_cpu.numpy(), images, segs, depths, has_attention_mask=True,
                                                 reserve=max_new_tokens, attention_mask=attention_mask)
            self.engine.clear_attention_mask()   # generate(): the cached steps run under an all-ones mask (:130-133)
            self._generation += 1
            logits = torch.from_numpy(last)
            unfinished = torch.ones(B, dtype=torch.long)
            cur = ids_cpu
            if generator is None and do_sample:
                generator = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
            lp_cols, top_lp_cols, top_id_cols = [], [], []
            alive = torch.ones(B, dtype=torch.bool)   # rows whose finishing token has not been emitted yet
            for step in range(max_new_tokens):
                scores = logits.float()
                raw = scores
                if gd is not None:   # the first processor of the list; the log-probs below stay those of the raw conditional rows
                    raw = scores[:B]
                    scores = _lp.apply_guidance(scores[:B], scores[B:], gscale)
                if proc is not None:   # in front of the warpers, as HF; the log-probs below stay those of `raw`
                    scores = _lp.apply_torch(proc, cur, scores, T, ([] if eos is None else [int(eos)]) + eos_more)
                if allowed_fn is not None:   # behind the processors (4.31's order); finished rows emit pad: not constrained
                    scores = _lp.apply_prefix_constraint(allowed_fn, cur, scores, skip=(unfinished == 0) if eos is not None else None)
                if do_sample:
                    scores = scores / float(temperature)
                    if top_k and 0 < top_k < scores.shape[-1]:
                        kth = torch.topk(scores, top_k)[0][..., -1, None]
                        scores = scores.masked_fill(scores < kth, float("-inf"))
                    if top_p is not None and top_p < 1.0:
                        scores = _top_p_filter(scores, float(top_p))
                    if any(warp):
                        scores = _lp.apply_warpers(scores, *warp)
                    probs = torch.softmax(scores, dim=-1)
                    nxt = torch.multinomial(probs, 1, generator=generator).squeeze(1)
                else:
                    nxt = torch.argmax(scores, dim=-1)
                if eos is not None:
                    nxt = nxt * unfinished + pad * (1 - unfinished)
                cur = torch.cat([cur, nxt[:, None]], dim=1)
                if want_lp:
                    # the raw distribution, as the device kernel: log_softmax of the fp32 logits; stable descending sort = ties to
                    # the lower id; entries that are -inf hold id -1; rows behind their finishing token 0.0 / 0.0 / -1
                    lsm = torch.log_softmax(raw, dim=-1)
                    col = lsm.gather(1, nxt[:, None]).squeeze(1)
                    lp_cols.append(torch.where(alive, col, torch.zeros_like(col)))
                    if K:
                        order = torch.sort(raw, dim=-1, descending=True, stable=True)[1][:, :K]
                        if order.shape[1] < K:
                            order = torch.cat([order, order.new_zeros(B, K - order.shape[1])], 1)
                        tl = lsm.gather(1, order)
                        tl[:, raw.shape[-1]:] = float("-inf")
                        ti = torch.where(torch.isinf(tl) & (tl < 0), torch.full_like(order, -1), order)
                        top_lp_cols.append(torch.where(alive[:, None], tl, torch.zeros_like(tl)))
                        top_id_cols.append(torch.where(alive[:, None], ti, torch.full_like(ti, -1)))
                    if eos is not None:
                        alive = alive & unfinished.bool() & ~torch.isin(nxt, torch.tensor([eos] + eos_more))
                if streamer is not None:
                    streamer.put(nxt.cpu())
                if eos is not None:
                    unfinished = unfinished * (~torch.isin(nxt, torch.tensor([eos] + eos_more))).long()
                stop = bool(unfinished.max() == 0) if eos is not None else False
                if stopping_criteria:
                    for crit in stopping_criteria:
                        r = crit(cur, scores)
                        stop = stop or bool(r.all() if hasattr(r, "all") else r)
                if stop or step + 1 == max_new_tokens:
                    break
                step_tok = nxt.numpy().astype(np.int32)
                lg, _ = self.engine.decode_step(np.concatenate([step_tok, step_tok]) if gd is not None else step_tok)
                logits = torch.from_numpy(lg)
            out = cur
            if want_lp:
                tok_lp = torch.stack(lp_cols, 1).float()
                top_lp = torch.stack(top_lp_cols, 1).float() if K else torch.zeros(B, tok_lp.shape[1], 0)
                top_id = torch.stack(top_id_cols, 1).to(torch.int64) if K else torch.zeros(B, tok_lp.shape[1], 0, dtype=torch.int64)
            if streamer is not None:
                streamer.end()
        if hasattr(input_ids, "device"):
            out = out.to(input_ids.device)
        if not as_dict:
            return out
        spec = self.engine.last_speculation
        if not want_lp:
            return GenerateOutput(sequences=out, speculation=spec)
        return GenerateOutput(sequences=out, token_logprobs=tok_lp, top_logprobs=top_lp if K else None,
                              top_token_ids=top_id if K else None, sequence_logprob=tok_lp.sum(dim=1), speculation=spec)

    _sample_calls = 0

    def _negative_prompt(self, input_ids, negative_prompt_ids, negative_prompt_attention_mask, negative_images, negative_segs,
                         negative_depths):
        """the negative prompt of a guided generate as [B, Tn] int64 numpy — HF's default (the last prompt token alone) without
        negative_prompt_ids; every refusal that needs no engine"""
        B = input_ids.shape[0]
        to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        if negative_prompt_ids is None:
            neg = to_np(input_ids)[:, -1:]
        else:
            neg = to_np(negative_prompt_ids)
            if neg.ndim != 2 or neg.shape[0] not in (1, B) or neg.shape[1] < 1:
                raise ValueError(f"`negative_prompt_ids` has to be [{B}, Tn] or [1, Tn], but is {tuple(neg.shape)}")
            if neg.shape[0] != B:
                neg = np.repeat(neg, B, axis=0)
        neg = np.ascontiguousarray(neg, dtype=np.int64)
        if negative_prompt_attention_mask is not None:
            mk = to_np(negative_prompt_attention_mask)
            if mk.ndim != 2 or mk.shape[1] != neg.shape[1] or mk.shape[0] not in (1, B):
                raise ValueError(f"`negative_prompt_attention_mask` has to match negative_prompt_ids, but is {tuple(mk.shape)}")
            if not bool(np.all(mk != 0)):
                if negative_images is None:
                    raise NotImplementedError("a padded TEXT-ONLY batch (attention_mask with zeros, images=None) is outside the "
                                              "VCoder hot path")
                raise ValueError("`negative_prompt_ids` has to be rectangular and unpadded: its attention mask holds zeros")
        s = self.engine.cfg.vit_image_size
        for name, a in (("negative_images", negative_images), ("negative_segs", negative_segs), ("negative_depths", negative_depths)):
            if a is not None and tuple(a.shape) != (B, 3, s, s):
                raise ValueError(f"`{name}` has to be [{B}, 3, {s}, {s}], but is {tuple(a.shape)}")
        if negative_images is None and (negative_segs is not None or negative_depths is not None):
            raise ValueError("`negative_segs` / `negative_depths` need `negative_images`")
        if bool((neg < 0).any()):
            if negative_images is None:
                raise ValueError("`negative_prompt_ids` holds image placeholders, but no `negative_images` were given")
            from ..constants import DEPTH_TOKEN_INDEX, SEG_TOKEN_INDEX
            if bool((neg == SEG_TOKEN_INDEX).any()) and self.variant != "llava" and negative_segs is None:
                raise ValueError("`negative_prompt_ids` holds seg placeholders, but no `negative_segs` were given")
            if bool((neg == DEPTH_TOKEN_INDEX).any()) and self.variant == "vcoder_ds" and negative_depths is None:
                raise ValueError("`negative_prompt_ids` holds depth placeholders, but no `negative_depths` were given")
        return neg

    # ---- beam search (HF GenerationMixin.beam_search + BeamSearchScorer of the reference's pinned Transformers 4.31) -----------
    def _beam_search_device(self, input_ids, images, segs, depths, num_beams, max_new_tokens, max_length, eos_token_id, pad_token_id,
                            attention_mask, length_penalty, early_stopping, len_counts_prompt):
        """generate(num_beams=n) through HipEngine.generate_beam: the whole loop of `_beam_search` below on the device (one
        captured beam step per token, scores in fp32), its finalisation in the engine.  -> ([B, T + L] int64 in the form
        `_beam_search` returns, sequences_scores [B] float32)."""
        import torch

        ids_cpu = input_ids.detach().cpu() if hasattr(input_ids, "detach") else torch.as_tensor(np.asarray(input_ids))
        T = ids_cpu.shape[1]
        if max_new_tokens is None:
            max_new_tokens = (max_length - T) if max_length is not None else 20
        eos = self.config.eos_token_id if eos_token_id is None else eos_token_id
        eos_list = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else ([] if eos is None else [eos])) if int(e) >= 0]
        pad = pad_token_id if pad_token_id is not None else (self.config.pad_token_id if self.config.pad_token_id is not None
                                                             else (eos_list[0] if eos_list else None))
        segs = segs if self.variant != "llava" else None
        depths = depths if self.variant == "vcoder_ds" else None
        new, _, scores = self.engine.generate_beam(ids_cpu.numpy(), images, segs, depths, num_beams=num_beams,
                                                   max_new_tokens=max_new_tokens, eos_token_id=eos_list or None, pad_token_id=pad,
                                                   length_penalty=length_penalty, early_stopping=early_stopping,
                                                   len_counts_prompt=len_counts_prompt, attention_mask=attention_mask)
        self._generation += 1
        out = torch.cat([ids_cpu, torch.from_numpy(new.astype(np.int64))], dim=1)
        if hasattr(input_ids, "device"):
            out = out.to(input_ids.device)
        return out, torch.from_numpy(scores)

    def _beam_search(self, input_ids, images, segs, depths, num_beams, max_new_tokens, max_length, eos_token_id, pad_token_id,
                     attention_mask, stopping_criteria, length_penalty, early_stopping, len_counts_prompt, sample=None,
                     return_scores=False, processors=None, allowed_fn=None):
        """`generate(num_beams=n)` as the reference's eval loaders can ask for it (eval/model_seg_loader.py:129-139 forwards
        args.num_beams): every sequence is expanded to n beams (rows b*n .. b*n+n-1, as `_expand_inputs_for_generation`), the
        prefill and one cached decode step per token run on the engine, scoring is HF's — log-softmax of the fp32 logits plus
        the running beam score, the 2n best continuations per sequence, BeamSearchScorer.process / finalize (hypotheses
        scored by sum_logprobs / len ** length_penalty; 4.31 counts the PROMPT ids in len) — and the KV rows are reordered by
        beam_idx after every step (vc_reorder_cache).  Returns [B, T + n_new] int64, shorter rows padded with pad_token_id
        (after one EOS), like HF.

        sample (do_sample=True: `beam_sample` of Transformers 4.31, generation/utils.py): the 2n candidates per sequence are DRAWN
        instead of taken — the warpers (temperature -> top-k -> top-p) act on log-softmax + running beam score, as 4.31 applies
        them, `torch.multinomial(softmax(.), 2n)` over the n * V continuations, the draws sorted by score — everything behind it
        (EOS handling, hypotheses, cache reorder) is the beam search's.  The draws come from the caller's torch generator
        (or `seed`), so a seed reproduces them; bit-equality with a given HF version's stream is not defined (its warper
        order changed after 4.31).

        processors (logits_processors.LogitsProcessors): applied to log_softmax(logits) over every beam row's ids before the running
        beam score is added, as 4.31's beam_search / beam_sample apply their logits_processor.  allowed_fn (a
        prefix_allowed_tokens_fn): PrefixConstrainedLogitsProcessor behind them, fn(row // num_beams, ids of the beam row); the rows
        of a sequence that is done are skipped (their tokens are pad)."""
        import torch

        ids_cpu = input_ids.detach().cpu() if hasattr(input_ids, "detach") else torch.as_tensor(np.asarray(input_ids))
        B, T = ids_cpu.shape
        nb = num_beams
        if B * nb > self.engine.MAX_BATCH:
            raise ValueError(f"batch {B} x num_beams {nb} exceeds the {self.engine.MAX_BATCH} rows a replica decodes at a time")
        if max_new_tokens is None:
            max_new_tokens = (max_length - T) if max_length is not None else 20
        eos = self.config.eos_token_id if eos_token_id is None else eos_token_id
        # an int or a list of ids (HF's BeamSearchScorer takes both and tests membership); negative = none
        eos_list = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else ([] if eos is None else [eos])) if int(e) >= 0]
        eos_set = set(eos_list)
        eos = eos_list[0] if eos_list else None          # what pads / terminates a finished row (HF: eos_token_id[0])
        pad = pad_token_id if pad_token_id is not None else (self.config.pad_token_id if self.config.pad_token_id is not None else eos)
        segs = segs if self.variant != "llava" else None
        depths = depths if self.variant == "vcoder_ds" else None
        rep = np.repeat(np.arange(B), nb)

        def expand(a):
            if a is None:
                return None
            if isinstance(a, (list, tuple)):
                return [a[i] for i in rep]
            return a[torch.as_tensor(rep, device=a.device)] if hasattr(a, "detach") else np.asarray(a)[rep]

        ids_x = ids_cpu[torch.as_tensor(rep)]
        mask_x = expand(attention_mask)
        last, _, S = self.engine.prefill(ids_x.numpy(), expand(images), expand(segs), expand(depths), has_attention_mask=True,
                                         reserve=max_new_tokens, attention_mask=mask_x)
        self.engine.clear_attention_mask()          # cached steps under the all-ones mask (vcoder_ds_llava_arch.py:130-133)
        self._generation += 1
        V = last.shape[-1]
        seqs = ids_x.clone()                                                  # [B*nb, T + generated]
        beam_scores = torch.zeros(B, nb)
        beam_scores[:, 1:] = -1e9
        beam_scores = beam_scores.view(-1)
        hyps = [[] for _ in range(B)]                                         # per sequence: (score, ids), at most nb kept
        worst = [1e9] * B
        done = [False] * B

        def hyp_len(n_ids):                                                    # 4.31: the whole id row; >= 4.38: generated part only
            return n_ids if len_counts_prompt else n_ids - T

        def add_hyp(b, ids_row, sum_logprobs):
            score = sum_logprobs / (max(hyp_len(ids_row.shape[-1]), 1) ** length_penalty)
            if len(hyps[b]) < nb or score > worst[b]:
                hyps[b].append((score, ids_row))
                if len(hyps[b]) > nb:
                    srt = sorted((s_, i) for i, (s_, _) in enumerate(hyps[b]))
                    del hyps[b][srt[0][1]]
                    worst[b] = srt[1][0]
                else:
                    worst[b] = min(score, worst[b])

        def is_done(b, best_sum_logprobs, cur_len):
            if len(hyps[b]) < nb:
                return False
            if early_stopping is True:
                return True
            if early_stopping is False:
                return worst[b] >= best_sum_logprobs / (max(hyp_len(cur_len), 1) ** length_penalty)
            # "never"
            hl = hyp_len(cur_len) if length_penalty <= 0.0 else hyp_len(T + max_new_tokens)
            return worst[b] >= best_sum_logprobs / (max(hl, 1) ** length_penalty)

        logits = torch.from_numpy(last).float()
        n_steps = 0
        for step in range(max_new_tokens):
            scores = torch.log_softmax(logits, dim=-1)
            if processors is not None:
                scores = _lp.apply_torch(processors, seqs, scores, T, eos_list)
            if allowed_fn is not None:
                scores = _lp.apply_prefix_constraint(allowed_fn, seqs, scores, nb, skip=[done[r // nb] for r in range(B * nb)])
            scores = scores + beam_scores[:, None]
            if sample is not None:
                w = scores / sample["temperature"]
                if 0 < sample["top_k"] < V:
                    kth = torch.topk(w, sample["top_k"])[0][..., -1, None]
                    w = w.masked_fill(w < kth, float("-inf"))
                if sample["top_p"] < 1.0:
                    w = _top_p_filter(w, sample["top_p"], min_tokens_to_keep=2)   # 4.31: min_tokens_to_keep = 2 when num_beams > 1
                if any(sample.get("warp", ())):
                    w = _lp.apply_warpers(w, *sample["warp"], min_tokens_to_keep=2)
                flat = w.view(B, nb * V)
                probs = torch.softmax(flat, dim=-1)
                # torch.multinomial without replacement needs >= 2n non-zero entries (step 0: only beam 0 is alive, and a tight
                # top_p / top_k can leave fewer): the finite-score continuations are topped up with the next-best ones by score
                short = (probs > 0).sum(-1) < 2 * nb
                if bool(short.any()):
                    fill = torch.topk(scores.view(B, nb * V), 2 * nb, dim=1).indices
                    tiny = torch.zeros_like(probs).scatter(1, fill, torch.finfo(probs.dtype).tiny)
                    probs = torch.where(short[:, None] & (probs == 0), tiny, probs)
                    flat = torch.where(short[:, None] & torch.isinf(flat) & (tiny > 0), scores.view(B, nb * V), flat)
                draw = torch.multinomial(probs, 2 * nb, generator=sample["generator"])
                top_s, order = torch.sort(torch.gather(flat, -1, draw), descending=True, dim=1)
                top_i = torch.gather(draw, -1, order)
                scores = w
            else:
                top_s, top_i = torch.topk(scores.view(B, nb * V), 2 * nb, dim=1, largest=True, sorted=True)
            next_idx, next_tok = top_i // V, top_i % V
            nscore, ntok, nsrc = torch.zeros(B, nb), torch.zeros(B, nb, dtype=torch.long), torch.zeros(B, nb, dtype=torch.long)
            cur_len = seqs.shape[1]
            for b in range(B):
                if done[b]:
                    ntok[b] = pad if pad is not None else 0
                    continue
                k = 0
                for rank in range(2 * nb):
                    tok, sc, src = int(next_tok[b, rank]), float(top_s[b, rank]), b * nb + int(next_idx[b, rank])
                    if tok in eos_set:
                        if rank >= nb:
                            continue
                        add_hyp(b, seqs[src].clone(), sc)
                    else:
                        nscore[b, k], ntok[b, k], nsrc[b, k] = sc, tok, src
                        k += 1
                    if k == nb:
                        break
                if k < nb:
                    raise ValueError(f"At most {nb} tokens in {next_tok[b].tolist()} can be equal to `eos_token_id: {eos}`.")
                done[b] = done[b] or is_done(b, float(top_s[b].max()), cur_len)
            beam_scores = nscore.view(-1)
            beam_idx = nsrc.view(-1)
            seqs = torch.cat([seqs[beam_idx], ntok.view(-1, 1)], dim=1)
            n_steps = step + 1
            stop = all(done)
            if stopping_criteria:
                for crit in stopping_criteria:
                    r = crit(seqs, scores)
                    stop = stop or bool(r.all() if hasattr(r, "all") else r)
            if stop or step + 1 == max_new_tokens:
                break
            self.engine.reorder_cache(beam_idx.numpy())
            lg, _ = self.engine.decode_step(ntok.view(-1).numpy().astype(np.int32))
            logits = torch.from_numpy(lg).float()
        # finalize: open beams become hypotheses, the best one per sequence is returned
        out_rows, best_scores = [], []
        for b in range(B):
            if not done[b]:
                for j in range(nb):
                    add_hyp(b, seqs[b * nb + j], float(beam_scores[b * nb + j]))
            best_score, best_row = max(hyps[b], key=lambda t_: t_[0])
            out_rows.append(best_row)
            best_scores.append(best_score)
        L = max(r.shape[0] for r in out_rows)
        max_len = T + max_new_tokens
        L_out = min(L + 1, max_len)            # BeamSearchScorer.finalize: room for the EOS a finished hypothesis does not carry
        if any(r.shape[0] < L_out for r in out_rows) and pad is None:
            raise ValueError("`pad_token_id` has to be defined")
        out = torch.full((B, L_out), int(pad) if pad is not None else 0, dtype=torch.long)
        for b, r in enumerate(out_rows):
            out[b, : r.shape[0]] = r
            if r.shape[0] < L_out and eos is not None:
                out[b, r.shape[0]] = int(eos)
        if hasattr(input_ids, "device"):
            out = out.to(input_ids.device)
        return (out, torch.tensor(best_scores, dtype=torch.float32)) if return_scores else out


def _all_ones(attention_mask) -> bool:
    m = attention_mask.detach().cpu().numpy() if hasattr(attention_mask, "detach") else np.asarray(attention_mask)
    return bool(np.all(m != 0))


def _reference_keyword_stop(crit):
    """The reference's own KeywordsStoppingCriteria object (vcoder_llava/mm_utils.py:128-151): usable on the device when
    every keyword is ONE special token — its text check decodes with skip_special_tokens=True and can never match one, and
    its id check only works for single-token keywords in the first place.  Anything else -> None (host loop)."""
    kws, tok = getattr(crit, "keyword_ids", None), getattr(crit, "tokenizer", None)
    if kws is None or tok is None or not hasattr(crit, "keywords"):
        return None
    special = set(getattr(tok, "all_special_ids", []) or [])
    out = []
    for k in kws:
        ids = [int(t) for t in (k.tolist() if hasattr(k, "tolist") else k)]
        if len(ids) != 1 or ids[0] not in special:
            return None
        out.append(ids)
    return out


def _top_p_filter(scores, top_p: float, min_tokens_to_keep: int = 1):
    import torch

    s, idx = torch.sort(scores, descending=False, dim=-1)
    cum = s.softmax(-1).cumsum(-1)
    remove = cum <= (1 - top_p)
    remove[..., -min_tokens_to_keep:] = False
    mask = remove.scatter(1, idx, remove)
    return scores.masked_fill(mask, float("-inf"))


class LlavaLlamaForCausalLM(_HipCausalLMBase):
    variant, model_type = "llava", "llava"


class VCoderLlavaLlamaForCausalLM(_HipCausalLMBase):
    variant, model_type = "vcoder", "vcoder_llava"


class VCoderDSLlavaLlamaForCausalLM(_HipCausalLMBase):
    variant, model_type = "vcoder_ds", "vcoder_ds_llava"


class LlavaConfig(VCoderConfig):
    def __init__(self, **kw):
        kw.setdefault("variant", "llava")
        super().__init__(**kw)


class VCoderLlavaConfig(VCoderConfig):
    def __init__(self, **kw):
        kw.setdefault("variant", "vcoder")
        super().__init__(**kw)


class VCoderDSLlavaConfig(VCoderConfig):
    def __init__(self, **kw):
        kw.setdefault("variant", "vcoder_ds")
        super().__init__(**kw)
