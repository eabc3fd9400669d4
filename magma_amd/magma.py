"""Magma -- drop-in for reference magma/magma.py on MI355X.

Same public surface: ``Magma(config, device)``, ``from_checkpoint``,
``preprocess_inputs``, ``embed``, ``forward``, ``generate``, ``add_adapters``
and the attributes callers read (tokenizer, config, transforms, seq_len,
image_prefix, lm, word_embedding, transformer, image_token, eos_token, device).
The module tree keeps the reference's parameter names; the arithmetic runs in
libmagma_hip.so.  Differences: weights are created directly on the
GPU in bf16 (the reference builds fp32 on the CPU, then .half()); ``device``
must be a GPU -- there is no CPU execution path; SURVEY Q2 ("freeze_lm" as the
paper intends: only adapters, the image encoder and the prefix train)."""
from __future__ import annotations

from copy import deepcopy
from os.path import exists
from pathlib import Path
import os
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from .adapters import Adapter, AdapterWrapper, ParallelAdapter, ParallelAdapterWrapper
from .config import MultimodalConfig
from .image_input import ImageInput
from .image_prefix import ImagePrefix
from .language_model import GPTJConfig, LMOutput, get_gptj
from .sampling import generate
from .tokenizer import HeadSizedTokenizer
from .transforms import get_transforms
from .utils import build_labels, get_tokenizer, print_main


def _load_checkpoint_file(path):
    """torch.load to host memory: the safe unpickler first, the reference's full unpickle (magma.py:292) only on opt-in."""
    import argparse
    import pickle
    safe = [argparse.Namespace]
    try:      # numpy scalars (DeepSpeed's step counters): the reconstructor, numpy.dtype and the dtype classes it is called with
        import numpy as np
        safe += [np.dtype, np.ndarray]
        safe += [c for c in vars(getattr(np, "dtypes", None) or object()).values() if isinstance(c, type)]
        for mod in ("numpy._core.multiarray", "numpy.core.multiarray"):
            try:
                m = __import__(mod, fromlist=["scalar"])
                safe += [m.scalar, m._reconstruct]
                break
            except Exception:
                continue
    except Exception:
        pass
    try:
        with torch.serialization.safe_globals(safe):
            return torch.load(path, map_location=torch.device("cpu"), weights_only=True)
    except pickle.UnpicklingError as e:
        if os.environ.get("MAGMA_UNSAFE_UNPICKLE") != "1":
            raise RuntimeError(
                f"checkpoint {path} needs a full (code-executing) unpickle: {str(e).splitlines()[0]}  Set "
                "MAGMA_UNSAFE_UNPICKLE=1 to load it the way the reference does (torch.load without weights_only) -- only "
                "for files you trust.") from e
        import warnings
        warnings.warn(f"MAGMA_UNSAFE_UNPICKLE=1: loading {path} with a full unpickle", RuntimeWarning)
        return torch.load(path, map_location=torch.device("cpu"), weights_only=False)


class Magma(nn.Module):
    def __init__(self, config, device=None, lm_config: Optional[GPTJConfig] = None, enc: nn.Module = None,
                 dtype=torch.bfloat16, init_seed: Optional[int] = None):
        super().__init__()
        if isinstance(config, (str, Path)):
            config = MultimodalConfig.from_yml(config)
        else:
            assert isinstance(config, MultimodalConfig)
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        if self.device.type != "cuda":
            from .lib import MagmaHipError
            raise MagmaHipError("magma_amd.Magma runs on MI355X only (device=%s requested): pass device='cuda:0' (the "
                                "reference README's own call, Magma.from_checkpoint(..., device='cuda:0')); there is no CPU "
                                "execution path -- the CPU restatement lives in oracle/ and is test-only" % self.device)
        # every kernel launches on the CURRENT HIP device / stream (ops._need_gpu refuses operands that live elsewhere):
        # the model's device becomes current here and again in the entry points below
        torch.cuda.set_device(self.device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.config = config
        self.dtype = dtype
        self.lm = get_gptj(device=self.device, dtype=dtype, config=lm_config, init=True)
        if init_seed is not None:
            self.lm.init_weights(init_seed)
        self.seq_len = self.lm.config.max_position_embeddings
        self.tokenizer = get_tokenizer("gpt2", sequence_length=self.seq_len)
        self.image_token = self.tokenizer.cls_token_id
        self.eos_token = self.tokenizer.eos_token_id
        if lm_config is None:   # full-size model: len(tokenizer) = 50258
            self.lm.resize_token_embeddings(len(self.tokenizer))
        elif min(self.lm.config.vocab_size, self.lm.config.head_rows) < len(self.tokenizer):
            # reduced test vocabularies: keep the special ids in range of BOTH tables (eos = V-2, image = V-1)
            v = min(self.lm.config.vocab_size, self.lm.config.head_rows)
            self.eos_token, self.image_token = v - 2, v - 1
            # ... and what the tokenizer emits: its padding (GPT-2's eos, 50256) would otherwise be a label outside the head
            self.tokenizer = HeadSizedTokenizer(self.tokenizer, self.eos_token)
        self.lm.config.pad_token_id = self.tokenizer.eos_token_id
        self.word_embedding = self.lm.transformer.wte
        self.transformer = self.lm.transformer.h
        self.mlp_adapter_added, self.attn_adapter_added = False, False
        self.image_prefix = ImagePrefix(config=config, out_dim=self.lm.config.hidden_size, device=self.device,
                                        dtype=dtype, enc=enc)
        self.image_prefix_seq_len = self.image_prefix.out_seq_len
        # RGB images are resized / cropped / normalised on the GPU (bit-identical to the PIL host path of
        # reference transforms.py:121-134; MAGMA_HOST_PREPROCESS=1 keeps everything on the host)
        self.transforms = get_transforms(config.image_size, config.encoder_name,
                                         input_resolution=self.image_prefix.enc.input_resolution,
                                         device=None if os.environ.get("MAGMA_HOST_PREPROCESS") == "1" else self.device)
        if config.adapter_config:
            mlp_config = deepcopy(config.adapter_config.get("mlp", None))
            if mlp_config:
                assert mlp_config.get("adapter_type") is not None
                self.add_adapters(location="mlp", adapter_type=mlp_config.pop("adapter_type"),
                                  downsample_factor=mlp_config.pop("downsample_factor", 4), **mlp_config)
            attn_config = deepcopy(config.adapter_config.get("attention", None))
            if attn_config:
                assert attn_config.get("adapter_type") is not None
                self.add_adapters(location="attention", adapter_type=attn_config.pop("adapter_type"), **attn_config)
        # trainable set: adapters + image encoder + proj/ln; LM frozen
        if config.freeze_lm:
            for name, p in self.lm.named_parameters():
                p.requires_grad = bool(config.adapter_config) and "adapter" in name
        if config.freeze_img_encoder:
            for p in self.image_prefix.enc.parameters():
                p.requires_grad = False

    # ------------------------------------------------------------ adapters
    def add_adapters(self, downsample_factor: int = 4, adapter_type: str = "normal", location: str = "mlp",
                     ff_attr: str = "mlp", attn_attr: str = "attn", **adapter_kwargs):
        assert adapter_type in ["normal", "parallel", "scaled_parallel"], \
            "adapter_type must be one of 'normal', 'parallel', or 'scaled_parallel'"
        assert location in ["mlp", "attention"], "location must be one of 'mlp' or 'attention'"
        parallel = adapter_type in ("parallel", "scaled_parallel")
        if (location == "mlp" and self.mlp_adapter_added) or (location == "attention" and self.attn_adapter_added):
            raise ValueError("Adapter layer already added")
        dim = self.lm.config.hidden_size
        kw = dict(device=self.device, dtype=self.dtype)
        for blk in self.transformer:
            if location == "mlp" and parallel:        # reference magma.py:129-136
                setattr(blk, ff_attr, ParallelAdapter(module=getattr(blk, ff_attr), dim=dim, downsample_factor=downsample_factor,
                                                      scaled=adapter_type == "scaled_parallel", **adapter_kwargs, **kw))
            elif location == "mlp":
                adpt = Adapter(dim=dim, downsample_factor=downsample_factor, **adapter_kwargs, **kw)
                setattr(blk, ff_attr, nn.Sequential(getattr(blk, ff_attr), adpt))
            elif parallel:                            # reference magma.py:154-161
                setattr(blk, attn_attr, ParallelAdapterWrapper(module=getattr(blk, attn_attr), dim=dim,
                                                               downsample_factor=downsample_factor,
                                                               scaled="scaled" in adapter_type, **adapter_kwargs, **kw))
            else:
                setattr(blk, attn_attr, AdapterWrapper(attn_block=getattr(blk, attn_attr), dim=dim,
                                                       downsample_factor=downsample_factor, **adapter_kwargs, **kw))
        if location == "mlp":
            self.mlp_adapter_added = True
        else:
            self.attn_adapter_added = True
        self.lm.invalidate_packed()

    def invalidate_packed(self):
        from .adapters import bump_weights_epoch
        bump_weights_epoch()
        self.lm.invalidate_packed()
        self.image_prefix.invalidate_packed()

    def resize_token_embeddings(self, *args, **kwargs):
        """GPTJForCausalLM.resize_token_embeddings, then ``word_embedding`` -- the alias of lm.transformer.wte the reference keeps
        (magma.py:52), and a state-dict key of its own -- points at the table that replaced the old one."""
        self.lm.resize_token_embeddings(*args, **kwargs)
        self.word_embedding = self.lm.transformer.wte
        return self.word_embedding

    def load_state_dict(self, state_dict, strict: bool = True):
        r = super().load_state_dict(state_dict, strict=strict)
        self.invalidate_packed()
        return r

    # -------------------------------------------------------------- inputs
    def preprocess_inputs(self, input_list: list, embed=True) -> List[torch.Tensor]:
        """Strings -> token ids, ImageInput -> normalised image tensor; mutates the
        caller's list in place exactly like the reference (magma.py:181-186)."""
        for i in range(len(input_list)):
            inp = input_list[i]
            if isinstance(inp, str):
                input_list[i] = self.tokenizer.encode(inp, return_tensors="pt")
            elif isinstance(inp, ImageInput):
                input_list[i] = inp.get_transformed_image(transform_fn=self.transforms)
            else:
                raise Exception(f"Invalid input type:{type(inp)}")
        return self.embed(input_list) if embed else input_list

    @torch.no_grad()
    def embed(self, inputs: List[torch.Tensor]) -> torch.Tensor:
        """2-D -> word embeddings, 4-D -> image prefix; written straight into one
        (b, s, d) buffer (replaces the torch.cat at reference magma.py:212)."""
        from . import ops
        torch.cuda.set_device(self.device)
        parts, total, B = [], 0, None
        for x in inputs:
            if x.ndim == 2:
                n = x.shape[1]
            elif x.ndim == 4:
                n = None
            else:
                raise ValueError(f"Expected 2d or 4d tensor, got {x.ndim}d")
            parts.append(n)
            B = x.shape[0] if B is None else B
            assert x.shape[0] == B, "all inputs must share the batch size"
        d = self.lm.config.hidden_size
        embs = []
        for x, n in zip(inputs, parts):
            if n is None:
                embs.append(self.image_prefix(x.to(self.device)))
                total += embs[-1].shape[1]
            else:
                embs.append(None)
                total += n
        out = torch.empty(B, total, d, dtype=self.dtype, device=self.device)
        off = 0
        for x, n, e in zip(inputs, parts, embs):
            if e is None:
                ops.embedding(x.to(self.device).contiguous(), self.lm.engine.wte, out, row_off=off)
                off += n
            else:
                out[:, off:off + e.shape[1]] = e
                off += e.shape[1]
        return out

    @torch.no_grad()
    def embed_batch(self, batch: List[list], drop_images: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """A batch of requests with prompts of different lengths: ``batch`` is a list of per-sample input lists, each
        element a str, an ImageInput or an already preprocessed tensor (batch dimension 1) as ``preprocess_inputs`` /
        ``embed`` take them.  Returns (embeddings (B, S_max, d), right-padded with zeros; lengths int64 [B]) -- the
        arguments of ``generate(embeddings, lengths=lengths)``.  The caller's lists are left as they are; every image of
        the batch goes through ONE image_prefix call.
        ``drop_images=True``: the same samples with every ImageInput / 4-D item left out (no image is transformed or encoded)
        -- the text-only negative prompt of ``generate(..., guidance_scale=, negative_embeddings=)``; a sample that is left
        without inputs raises ValueError."""
        from . import ops
        torch.cuda.set_device(self.device)
        if not batch:
            raise ValueError("embed_batch: empty batch")
        samples = []
        for sample in batch:
            items = []
            for inp in sample:
                if drop_images and (isinstance(inp, ImageInput) or (isinstance(inp, torch.Tensor) and inp.ndim == 4)):
                    continue
                if isinstance(inp, str):
                    inp = self.tokenizer.encode(inp, return_tensors="pt")
                elif isinstance(inp, ImageInput):
                    inp = inp.get_transformed_image(transform_fn=self.transforms)
                elif not isinstance(inp, torch.Tensor):
                    raise Exception(f"Invalid input type:{type(inp)}")
                if inp.ndim not in (2, 4):
                    raise ValueError(f"Expected 2d or 4d tensor, got {inp.ndim}d")
                if inp.shape[0] != 1:
                    raise ValueError(f"embed_batch takes one sample per list: batch dimension 1, got {tuple(inp.shape)}")
                items.append(inp)
            if not items:
                raise ValueError("embed_batch: a sample without inputs" + (" once its images are dropped" if drop_images and sample else ""))
            samples.append(items)
        images = [x for items in samples for x in items if x.ndim == 4]
        prefix = None
        if images:
            if any(x.shape != images[0].shape for x in images):
                raise ValueError("embed_batch: all images of a batch must share one shape (the transforms give a fixed size)")
            prefix = self.image_prefix(torch.cat([x.to(self.device) for x in images]))     # ONE call for the whole batch
        P = 0 if prefix is None else prefix.shape[1]
        lengths = torch.tensor([sum(P if x.ndim == 4 else x.shape[1] for x in items) for items in samples], dtype=torch.int64)
        d = self.lm.config.hidden_size
        out = torch.zeros(len(samples), int(lengths.max()), d, dtype=self.dtype, device=self.device)
        k = 0
        for b, items in enumerate(samples):
            off = 0
            for x in items:
                if x.ndim == 4:
                    out[b, off:off + P] = prefix[k]
                    k += 1
                    off += P
                else:
                    ops.embedding(x.to(self.device).contiguous(), self.lm.engine.wte, out[b:b + 1], row_off=off)
                    off += x.shape[1]
        return out, lengths

    @torch.no_grad()
    def generate(self, embeddings, max_steps: int = 100, temperature: float = 0.7, top_k: int = 0,
                 top_p: float = 0.9, decode: bool = True, stop_on_eos: bool = True, seed: int = None,
                 eos_check_every: int = None, lengths=None, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, num_return_sequences: int = 1, return_scores: bool = False, past_key_values=None,
                 return_past_key_values: bool = False, *, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                 min_new_tokens: int = 0, suppress_tokens=None, eos_token=None, stop_sequences=None, stop_per_row: bool = None,
                 return_finish: bool = False, sampler: str = "reference", min_p: float = 0.0, return_logprobs: bool = False,
                 top_logprobs: int = 0, constraint=None, guidance_scale: float = 1.0, negative_embeddings=None,
                 negative_lengths=None, guidance_min_p: float = 0.0, num_beam_groups: int = 1, diversity_penalty: float = 0.0,
                 penalty_alpha: float = 0.0, prompt_lookup_num_tokens: int = 0, max_matching_ngram_size: int = 2, lookup_ids=None,
                 return_speculation: bool = False):
        """reference magma.py:214-236 (+ stop_on_eos / seed / eos_check_every / lengths, see sampling.generate).
        ``lengths``: prompts of different lengths, right-padded (embed_batch); ``embeddings`` may also be a list of
        per-sample (1, s_i, d) tensors.  ``num_beams`` > 1: beam search (length_penalty, early_stopping,
        num_return_sequences, return_scores: see sampling.generate).  ``return_past_key_values=True`` returns (output, past);
        ``past_key_values=past`` continues that conversation with ``embeddings`` as the next turn (see sampling.generate).
        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_new_tokens`` / ``suppress_tokens``: transformers' logits
        processors of those names over the tokens this call generates, inside the token step (see sampling.generate).
        ``eos_token`` (None: the model's eos; an id or 1 to 8 ids) / ``stop_sequences`` (at most 16 token-id sequences or strings,
        matched over token ids) / ``stop_per_row`` / ``return_finish``: per-row stopping as in transformers -- a finished row is
        padded and stays finished, the call ends when every row is finished (see sampling.generate).
        ``sampler="transformers"``: temperature, top-k, nucleus top-p and ``min_p`` as transformers' warpers apply them, instead of
        the reference's filters (see sampling.generate).
        ``return_logprobs`` / ``top_logprobs`` (0 to 20 alternatives per token): a ``TokenLogprobs`` appended to the result -- every
        generated token's log-probability under the raw model distribution, as ``score`` gives it (see sampling.generate).
        ``constraint`` (a ``sampling.TokenTrie``, a list of token-id sequences or strings, or one of either per row): every row's
        output stays inside that closed set of answers, followed by eos (see sampling.generate; ``choose`` maps it back).
        ``guidance_scale`` (1.0 = off) / ``negative_embeddings`` (what ``embeddings`` takes; ``embed_batch(batch, drop_images=True)``
        gives the text-only prompt) / ``negative_lengths`` / ``guidance_min_p``: classifier-free guidance against a negative prompt
        -- transformers' ``guidance_scale`` / ``negative_prompt_ids`` rule with the plausibility cut of contrastive decoding, inside
        the token step; the output is laid out as for ``embeddings`` alone (see sampling.generate).
        ``num_beam_groups`` (a divisor of ``num_beams``) / ``diversity_penalty``: diverse beam search -- the beams run in groups
        that are penalised for selecting the tokens earlier groups selected at the same step, and ``num_return_sequences`` takes
        the groups' hypotheses round-robin: several different captions of one image (see sampling.generate).
        ``penalty_alpha`` in (0, 1] with ``top_k`` in [1, 16]: contrastive search -- among the ``top_k`` most probable tokens the one
        whose hidden state is least similar to the context's, deterministic (see sampling.generate).
        ``seed`` / ``temperature`` / ``top_k`` / ``top_p`` / ``min_p`` may each be a sequence of B values: every row then samples
        under its own settings and seed and equals its one-row call (see sampling.generate, per-row sampling).
        ``prompt_lookup_num_tokens`` = k in [1, 7] / ``max_matching_ngram_size`` / ``lookup_ids`` / ``return_speculation``:
        speculative decoding -- every step verifies k prompt-lookup drafts per row beside its newest token and keeps what the
        model agrees with; the output is the per-row greedy call's, token for token.  With ``temperature != 0`` (scalars stand for
        every row) or per-row settings it is seed-exact: row b equals ``generate(row_b, ..., seed=s_b)`` alone; ``stop_sequences``
        apply as in the plain call (see sampling.generate)."""
        torch.cuda.set_device(self.device)
        return generate(self, embeddings=embeddings, max_steps=max_steps, temperature=temperature, top_k=top_k,
                        top_p=top_p, decode=decode, stop_on_eos=stop_on_eos, seed=seed, eos_check_every=eos_check_every,
                        lengths=lengths, num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping,
                        num_return_sequences=num_return_sequences, return_scores=return_scores,
                        past_key_values=past_key_values, return_past_key_values=return_past_key_values,
                        repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                        min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens, eos_token=eos_token,
                        stop_sequences=stop_sequences, stop_per_row=stop_per_row, return_finish=return_finish, sampler=sampler,
                        min_p=min_p, return_logprobs=return_logprobs, top_logprobs=top_logprobs, constraint=constraint,
                        guidance_scale=guidance_scale, negative_embeddings=negative_embeddings, negative_lengths=negative_lengths,
                        guidance_min_p=guidance_min_p, num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty,
                        penalty_alpha=penalty_alpha, prompt_lookup_num_tokens=prompt_lookup_num_tokens,
                        max_matching_ngram_size=max_matching_ngram_size, lookup_ids=lookup_ids,
                        return_speculation=return_speculation)

    def generate_stream(self, requests, **kwargs):
        """Generate over a stream of requests -- an iterable of ``embed`` outputs, or pairs (embeddings, max_new_tokens) --: a
        generator of ``sampling.StreamResult(index, tokens, text, reason, reason_index, slot)``, one per request in completion
        order, each what a solo ``generate`` of that request gives.  The HIP engine hands the row of a finished request to the next
        one while the other rows keep generating (see sampling.generate_stream for the keywords).  ``per_request=True``: an item may
        be a ``sampling.StreamRequest`` with sampler settings and a seed of its own, reproducible against its solo call."""
        from .sampling import generate_stream
        torch.cuda.set_device(self.device)
        return generate_stream(self, requests, **kwargs)

    @torch.no_grad()
    def choose(self, embeddings, choices, lengths=None, **generate_kwargs):
        """Which of ``choices`` (a ``sampling.TokenTrie``, a list of token-id sequences or strings, or one of either per row) the
        model answers with: constrained GREEDY decoding (``generate(constraint=choices, temperature=0, return_logprobs=True)``,
        ``max_steps`` = the longest choice + 1).  Returns (index int64 [B]: the position of row b's answer in its choices,
        ``TokenLogprobs`` of the path under the raw distribution).  It follows the locally most probable allowed token; it is NOT
        the arg-max of the total sequence probability -- ``rank`` gives that, for all choices in one forward (see sampling.choose)."""
        from .sampling import choose
        torch.cuda.set_device(self.device)
        return choose(self, embeddings, choices, lengths=lengths, **generate_kwargs)

    def choose_stream(self, requests, **kwargs):
        """``choose`` over a stream of requests -- an iterable of pairs (``embed`` output, that request's choices) --: a generator
        of ``sampling.StreamChoice(index, choice, tokens, logprobs, top_ids, top_logprobs, reason, slot)``, one per request in
        completion order, each what a solo ``choose`` of that request gives.  The HIP engine runs them through the slots of a
        request stream: a short answer frees its row for the next request (see sampling.choose_stream for the keywords)."""
        from .sampling import choose_stream
        torch.cuda.set_device(self.device)
        return choose_stream(self, requests, **kwargs)

    @torch.no_grad()
    def rank(self, embeddings, choices, lengths=None, *, eos: bool = True, length_penalty: float = 0.0, max_nodes: int = None,
             return_terms: bool = False):
        """Rank ``choices`` (what ``choose`` takes) by their probability as whole sequences after the prompt ``embeddings`` /
        ``lengths`` (what ``generate`` takes): the closed-vocabulary evaluation of a captioning / VQA model (DESIGN.md "Ranking
        choices").  Returns ``sampling.Ranking(index int64 [B], scores fp32 [B, C], logprobs fp32 [B, C], count int64 [B, C])``,
        columns in the caller's order: ``logprobs[b, c]`` = sum_j log p(choice_c[j] | prompt_b, choice_c[:j]) + (``eos``)
        log p(eos | prompt_b, choice_c) under the raw distribution -- ``score``'s numbers --, ``count`` the number of terms,
        ``scores = logprobs / count ** length_penalty``, ``index`` the arg-max (lowest position on a tie); rows with fewer choices
        are padded with -inf / 0.  All choices of a row cost ONE forward over prompt + trie nodes (shared prefixes once), not one
        forward per candidate; ``max_nodes`` caps the nodes per forward (see sampling.rank)."""
        from .sampling import rank
        torch.cuda.set_device(self.device)
        return rank(self, embeddings, choices, lengths=lengths, eos=eos, length_penalty=length_penalty, max_nodes=max_nodes,
                    return_terms=return_terms)

    def _score_inputs(self, embeddings, targets, lengths=None, width: int = None, host_check=None):
        """What score() and explain() feed the engine: the checked prompts and targets as (emb (B, W, d) on the device = [prompt_b ;
        wte(targets_b[:-1])] right-padded with zeros, tgt (B, W) int64 host: the token position s of row b predicts or -100, tokens
        (B, T) int64 host right-padded with -100, count int64 [B], lens int64 [B], S = the prompts' padded width).  W = max_b (len_b + count_b - 1), or ``width``
        when that is larger.  ``host_check(B, W, S)`` runs after every check of the inputs and before the first launch."""
        from . import ops
        from .sampling import prompt_batch
        eng = self.lm.engine
        embeddings, lens = prompt_batch(embeddings, lengths)
        B, S, d = embeddings.shape
        if lens is None:
            lens = torch.full((B,), S, dtype=torch.int64)
        if torch.is_tensor(targets):
            t = targets.detach().to("cpu")
            if t.ndim != 2 or t.shape[0] != B or t.is_floating_point() or t.dtype == torch.bool:
                raise ValueError(f"targets must be integers of shape ({B}, T), got {t.dtype} {tuple(t.shape)}")
            rows = []
            for r in t.to(torch.int64).tolist():
                n = sum(1 for v in r if v != -100)
                if any(v == -100 for v in r[:n]):
                    raise ValueError("targets must be right-padded with -100 (an ignored position in front of a target)")
                rows.append(r[:n])
        else:
            if len(targets) != B:
                raise ValueError(f"{len(targets)} target rows for {B} prompts")
            rows = [[int(v) for v in (r.tolist() if torch.is_tensor(r) else r)] for r in targets]
        if any(len(r) < 1 for r in rows):
            raise ValueError("every row needs at least one target id")
        ops.refuse_targets_outside(torch.tensor([v for r in rows for v in r], dtype=torch.int64), eng.V)
        count = torch.tensor([len(r) for r in rows], dtype=torch.int64)
        total = lens + count - 1
        n_pos = self.lm.config.max_position_embeddings
        W, T = int(total.max()), int(count.max())
        if width is not None:
            if int(width) < W:
                raise ValueError(f"width {width} is less than the {W} positions the batch needs")
            W = int(width)
        if W > n_pos:
            raise ValueError(f"prompt plus targets reach {W} positions, beyond max_position_embeddings = {n_pos}")
        if host_check is not None:
            host_check(B, W, S)
        emb = torch.zeros(B, W, d, dtype=self.dtype, device=self.device)
        tgt = torch.full((B, W), -100, dtype=torch.int64)
        tokens = torch.full((B, T), -100, dtype=torch.int64)
        for b, r in enumerate(rows):
            L = int(lens[b])
            emb[b, :L] = embeddings[b, :L]
            if len(r) > 1:
                ops.embedding(torch.tensor([r[:-1]], dtype=torch.int64, device=self.device), eng.wte, emb[b:b + 1], row_off=L)
            tgt[b, L - 1: L - 1 + len(r)] = torch.tensor(r, dtype=torch.int64)
            tokens[b, : len(r)] = torch.tensor(r, dtype=torch.int64)
        return emb, tgt, tokens, count, lens, S

    @torch.no_grad()
    def score(self, embeddings, targets, lengths=None, *, top_logprobs: int = 0, key_scale=None, width: int = None,
              past_key_values=None):
        """How probable the model finds GIVEN tokens after a prompt (DESIGN.md "Token log-probabilities"): ranking candidate
        answers, per-caption perplexity (``exp(-logprobs.sum(1) / count)``).  ``embeddings`` is what ``generate`` takes as a
        prompt: (B, S, d) with optional ``lengths``, a list of per-sample tensors, or embed_batch's pair.  ``targets``: int64
        (B, T) right-padded with -100, or a list of id lists; at least one id per row, every id in [0, V).  One cache-less
        forward over [prompt_b ; wte(targets_b[:-1])], right-padded; the fp32 head runs only on the rows that predict a target.
        Returns a ``TokenLogprobs`` over the T columns: ``logprobs[b, j]`` = log p(targets_b[j] | prompt_b, targets_b[:j]) under
        the raw model distribution -- what ``generate(return_logprobs=True)`` reports for a token it selected --, the
        ``top_logprobs`` most probable tokens at every position, ``count[b]`` = the row's number of targets; positions past it
        hold 0.0 / -1 / -inf.  Scoring against a KV cache is not supported (``past_key_values`` raises NotImplementedError).

        ``key_scale`` (DESIGN.md "Explaining an answer"): scores under suppressed attention.  In every block and head the
        pre-softmax score of key j of row b is multiplied by key_scale[b, j]; 1.0 leaves a key alone, entries are finite and >= 0
        (checked on the host before any launch).  Shape (B, W) over the W = max_b (len_b + count_b - 1) positions of the forward,
        or (B, S) over the prompt positions only, which is right-padded with 1.0.  None launches what score always launched.
        ``width``: run the forward over this many positions (>= W; the extra ones are padding no row sees) -- what gives all
        forwards of ``explain`` one shape."""
        from .sampling import check_logprob_args, mask_logprobs
        torch.cuda.set_device(self.device)
        eng = self.lm.engine
        n_top = check_logprob_args(True, top_logprobs, eng.V)
        if past_key_values is not None:
            raise NotImplementedError("score runs one cache-less forward: past_key_values"
                                      + (" and key_scale are" if key_scale is not None else " is") + " not supported")
        if key_scale is not None and getattr(eng, "fp8_mode", False) and getattr(eng, "fp8_attn", False):
            raise NotImplementedError("key_scale is not implemented for the fp8 attention mode")
        scale = []

        def check_scale(B, W, S):           # on the host, before the first launch
            ks = torch.as_tensor(key_scale)
            if ks.ndim != 2 or ks.shape[0] != B or ks.shape[1] not in (W, S):
                raise ValueError(f"key_scale must have shape ({B}, {W}) or, over the prompt positions, ({B}, {S}); got {tuple(ks.shape)}")
            ks = eng.check_key_scale(ks, B, ks.shape[1])
            scale.append(ks if ks.shape[1] == W else torch.cat([ks, torch.ones(B, W - ks.shape[1])], 1))

        emb, tgt, tokens, count, lens, _ = self._score_inputs(embeddings, targets, lengths, width,
                                                              check_scale if key_scale is not None else None)
        B, T = tokens.shape
        key_scale = scale[0] if scale else None
        lp, top_id, top_lp = (v.cpu() for v in eng.score(emb, tgt, n_top, key_scale=key_scale))
        at = torch.arange(T)[None, :] < count[:, None]            # (b, j) order = the order of the kept rows
        out_lp, out_id, out_tl = torch.zeros(B, T), torch.zeros(B, T, n_top, dtype=torch.int64), torch.zeros(B, T, n_top)
        out_lp[at], out_id[at], out_tl[at] = lp, top_id.to(torch.int64), top_lp
        return mask_logprobs(tokens, out_lp, out_id, out_tl, count)

    @torch.no_grad()
    def explain(self, embeddings, targets, lengths=None, *, suppression: float = 0.9, units=None,
                similarity_threshold: float = None, batch_size: int = 16, return_terms: bool = False):
        """Which prompt positions carry an answer (DESIGN.md "Explaining an answer"): perturbation-only relevance by attention
        suppression (AtMan).  ``embeddings`` / ``lengths`` / ``targets`` are what ``score`` takes.  A unit is a set of prompt
        positions suppressed together -- by default one unit per prompt position; ``units``: per row a list of position lists (a
        word of several tokens, a block of patches).  For each unit the targets are scored again with the pre-softmax attention
        score of the unit's keys multiplied by ``1 - suppression`` in every block and head; the rise of the mean negative
        log-probability of the targets is the unit's relevance.  ``similarity_threshold`` = kappa: every prompt position whose
        embedding has cosine c >= kappa with one of the unit's is suppressed along with it, by ``1 - suppression * c``.
        Returns ``sampling.Explanation(relevance [B, U], loss [B], perturbed_loss [B, U], count [B])`` on the host; columns past
        count[b] hold 0.0; ``Explanation.grid`` cuts the image-patch map out of a row.  ``return_terms``: also the per-target
        log-probabilities, fp32 [B, 1 + U, T] (index 0: unperturbed; 0.0 where there is nothing).

        Cost: sum_b (1 + count[b]) rows, scored ``batch_size`` at a time in forwards of ONE shape (batch_size, W), W = max_b (len_b +
        n_targets_b - 1); the last forward is filled up with unperturbed copies.  A forward holds about 14 bf16 activations of
        batch_size x W x d elements (fused qkv | fc_in, q, k, v, V^T, the attention output, two residual streams) plus
        batch_size x n_targets fp32 logit rows of the padded vocabulary: 0.3 GB at batch_size 16, W 172, d 4096.  Whether that
        fits is the caller's business."""
        from .sampling import explain
        return explain(self, embeddings, targets, lengths=lengths, suppression=suppression, units=units,
                       similarity_threshold=similarity_threshold, batch_size=batch_size, return_terms=return_terms)

    @torch.no_grad()
    def cache_prompt(self, embeddings, lengths=None, cache_hint: int = 256):
        """A KV cache holding only the prompts ``embeddings`` ((B, S, d) with optional ``lengths``, a list of per-sample tensors,
        or embed_batch's (embeddings, lengths)), for ``generate(question, past_key_values=cache)``.  Shared prefix: cache one
        image and instruction once, then ``cache.expand(n)`` and ask n questions.  The cache belongs to the caller."""
        from .sampling import prompt_batch
        torch.cuda.set_device(self.device)
        embeddings, lens = prompt_batch(embeddings, lengths)
        if lens is None:
            lens = torch.full((embeddings.shape[0],), embeddings.shape[1], dtype=torch.int64)
        _, cache, _ = self.lm.engine.prefill(embeddings, cache_hint, lengths=lens)
        cache.set_rows(lens)
        return cache

    # ------------------------------------------------------------- forward
    def forward(self, images=None, captions=None, output_hidden_states: bool = False, input_embeddings=None,
                dropout_mask=None, return_logits: bool = False) -> LMOutput:
        """reference magma.py:238-276.  ``.loss`` and ``.logits`` (B, seq_len, V) bf16 as in the reference; the loss head runs
        on the rows that carry a target and the full logits tensor (2048 x 50258 per sample) is computed when a caller first
        reads ``.logits`` (or at once with ``return_logits=True``)."""
        torch.cuda.set_device(self.device)
        assert captions is not None, "Must provide captions in training"
        assert (images is None) != (input_embeddings is None), "Pass in either images, or input embeddings, not both."
        assert captions.shape[1] == self.seq_len, \
            f"in training, captions should be padded to sequence length ({self.seq_len}), but are length {captions.shape[1]}"
        from . import ops
        captions = captions.to(self.device).contiguous()
        if input_embeddings is None:
            input_embeddings = self.image_prefix(images.to(self.device), dropout_mask=dropout_mask)
        P = input_embeddings.shape[1]
        labels = build_labels(input_embeddings, captions, self.eos_token, self.device)
        B, S = captions.shape
        emb = torch.empty(B, S, self.lm.config.hidden_size, dtype=self.dtype, device=self.device)
        emb[:, :P] = input_embeddings
        ops.embedding(captions[:, : S - P].contiguous(), self.lm.engine.wte, emb, row_off=P)
        out = self.lm(inputs_embeds=emb, labels=labels, output_hidden_states=output_hidden_states,
                      return_logits=return_logits)
        out["labels"] = labels
        return out

    # ---------------------------------------------------------- checkpoints
    @classmethod
    def from_checkpoint(cls, config_path, checkpoint_path, device="cpu", **model_kwargs):
        """Load a (DeepSpeed-layout) MAGMA checkpoint: a torch-saved dict, optionally
        wrapped in "module" (reference magma.py:278-301).  The download fallback of
        the reference needs the network and is not reproduced.

        The signature is the reference's, default ``device='cpu'`` included (magma.py:279).  This build has no CPU
        execution path, so the default RAISES ``MagmaHipError`` naming the fix: pass ``device='cuda:0'`` as the
        reference's README does.  (The checkpoint itself is always read to host memory first, as in the reference.)

        The file is read with ``weights_only=True`` first (argparse.Namespace allow-listed: DeepSpeed's
        mp_rank_00_model_states.pt carries one next to "module").  A file that still needs a full unpickle -- which can
        execute arbitrary code -- is only loaded that way with ``MAGMA_UNSAFE_UNPICKLE=1`` (what the reference's call,
        written for torch < 2.6, always did)."""
        if not exists(checkpoint_path):
            raise FileNotFoundError(f"checkpoint {checkpoint_path} does not exist (no network download in this build)")
        model = cls(config=config_path, device=device, **model_kwargs)     # model_kwargs: reduced lm_config / enc (tests)
        from .tokenizer import ByteTokenizer
        if isinstance(getattr(model.tokenizer, "tok", model.tokenizer), ByteTokenizer) and os.environ.get("MAGMA_ALLOW_BYTE_TOKENIZER") != "1":
            raise RuntimeError("from_checkpoint needs the real GPT-2 tokenizer (set MAGMA_TOKENIZER_DIR to its files): the "
                               "byte-level stand-in would feed the wrong token ids to trained weights.  "
                               "MAGMA_ALLOW_BYTE_TOKENIZER=1 overrides (synthetic checkpoints / tests).")
        sd = _load_checkpoint_file(checkpoint_path)
        if "module" in sd.keys():
            sd = sd["module"]
        print_main(f"loading magma checkpoint from: {checkpoint_path}")
        missing, unexpected = model.load_checkpoint_state(sd)
        if missing:
            print_main(f"checkpoint has no value for {len(missing)} tensors (kept at their initial values): {missing[:8]}...")
        if unexpected:
            print_main(f"checkpoint keys without a destination: {unexpected[:8]}...")
        print_main("magma successfully loaded")
        model.eval()
        return model

    def load_checkpoint_state(self, sd: dict):
        """strict=False load that tolerates the reference's aliases (SURVEY Q8:
        ``transformer.N...`` / ``word_embedding.weight`` duplicate ``lm.transformer...``),
        skips buffers of the fork (attention.bias / masked_bias) and sniffs the
        vocabulary rows of wte / lm_head (Q1)."""
        own = self.state_dict()
        fixed = {}
        for k, v in sd.items():
            if k.endswith("attention.bias") or k.endswith("masked_bias"):
                continue
            if k.startswith("transformer."):       # alias of lm.transformer.h (reference magma.py:53)
                k = "lm.transformer.h." + k[len("transformer."):]
            elif k == "word_embedding.weight":
                k = "lm.transformer.wte.weight"
            fixed[k] = v
        # Q1: the input and the output vocabulary are sniffed independently (a checkpoint may carry a 50258-row wte next
        # to a 50400-row lm_head, or the reverse of neither)
        v_in = fixed["lm.transformer.wte.weight"].shape[0] if "lm.transformer.wte.weight" in fixed else None
        v_out = fixed["lm.lm_head.weight"].shape[0] if "lm.lm_head.weight" in fixed else None
        cur_in, cur_out = own["lm.transformer.wte.weight"].shape[0], own["lm.lm_head.weight"].shape[0]
        if (v_in is not None and v_in != cur_in) or (v_out is not None and v_out != cur_out):
            self.resize_token_embeddings(v_in if v_in is not None else cur_in, new_head_rows=v_out if v_out is not None else cur_out)
            own = self.state_dict()
        missing, unexpected = [], []
        bad = [f"{k}: checkpoint {tuple(v.shape)} vs model {tuple(own[k].shape)}" for k, v in fixed.items()
               if k in own and own[k].shape != v.shape]
        if bad:     # load_state_dict(strict=False) raises on a size mismatch too (reference magma.py:298)
            raise RuntimeError("size mismatch while loading the checkpoint: " + "; ".join(bad[:6]))
        with torch.no_grad():
            for k, v in fixed.items():
                if k in own:
                    # cast on the destination device (a 28-block fp32 checkpoint converts in ~1 s on the GPU, ~40 s on the host)
                    own[k].copy_(v.to(own[k].device).to(own[k].dtype))
                else:
                    unexpected.append(k)
        # the aliases of Q8 and BatchNorm's step counters are not "missing"
        missing = [k for k in own if k not in fixed and not k.endswith("num_batches_tracked")
                   and not k.startswith(("transformer.", "word_embedding."))]
        self.invalidate_packed()
        return missing, unexpected
