"""Autoregressive sampling loop -- behaviour of reference magma/sampling.py:43-121
(prefill on embeddings, then one token per step with the KV cache handed back;
greedy when temperature == 0.0; temperature / top-k / the reference's own
top-p filter otherwise; early stop when every row emitted EOS).

Differences: token selection -- greedy argmax AND the sampled branch --
runs as HIP kernels inside the captured token step (csrc/sampling.hip); the
per-step ``(next_token == eos).all()`` host sync of the reference (:109) became
a device-side record read every few steps.  ``top_k_filter`` / ``top_p_filter``
below are the host statements of the same rules (pinned to the reference's own
functions, tests/test_oracle_pins.py) and serve LM objects other than the engine."""
import os
from typing import List, Tuple, Union

import torch
import torch.nn.functional as F


def top_p_filter(logits, threshold: float = 0.9):
    """The reference's own "nucleus" rule, kept literally: sort descending, mark the
    ranks whose cumulative probability is still below ``1 - threshold``, shift that mark one rank to
    the right, never drop rank 0 -- which is NOT textbook top-p (it is usually a no-op)."""
    ranked, order = torch.sort(logits, descending=True)
    below = torch.cumsum(F.softmax(ranked, dim=-1), dim=-1) < (1 - threshold)
    drop = torch.zeros_like(below)
    drop[..., 1:] = below[..., :-1]
    ranked = ranked.masked_fill(drop, float("-inf"))
    return ranked.scatter(1, order, ranked)


def top_k_filter(logits, k):
    """Keep the k largest logits of every row, -inf elsewhere."""
    assert k > 0
    kept_val, kept_idx = torch.topk(logits, k)
    return torch.full_like(logits, float("-inf")).scatter_(1, kept_idx, kept_val)


def remove_tokens_after_eos(tensor, eos_token, image_token):
    """Everything from the first EOS on becomes EOS; image placeholders and EOS are then dropped."""
    hits = (tensor == eos_token).nonzero()
    if hits.any():
        tensor[hits[0]:] = eos_token
    return [tok for tok in tensor.tolist() if tok not in (image_token, eos_token)]


def pad_ragged(embeddings) -> Tuple[torch.Tensor, torch.Tensor]:
    """A list of per-sample embeddings ((1, s_i, d) or (s_i, d)) -> (right-padded (B, max s_i, d) with zero padding,
    lengths int64 [B] on the host)."""
    rows = []
    for e in embeddings:
        if e.ndim == 3:
            if e.shape[0] != 1:
                raise ValueError(f"a per-sample embedding must be (1, s, d) or (s, d), got {tuple(e.shape)}")
            e = e[0]
        elif e.ndim != 2:
            raise ValueError(f"a per-sample embedding must be (1, s, d) or (s, d), got {tuple(e.shape)}")
        if e.shape[0] < 1:
            raise ValueError("a per-sample embedding needs at least one position")
        rows.append(e)
    if not rows:
        raise ValueError("empty batch")
    d = rows[0].shape[1]
    if any(r.shape[1] != d or r.dtype != rows[0].dtype or r.device != rows[0].device for r in rows):
        raise ValueError("per-sample embeddings must share d, dtype and device")
    lengths = torch.tensor([r.shape[0] for r in rows], dtype=torch.int64)
    out = torch.zeros(len(rows), int(lengths.max()), d, dtype=rows[0].dtype, device=rows[0].device)
    for i, r in enumerate(rows):
        out[i, : r.shape[0]] = r
    return out, lengths


@torch.no_grad()
def generate(model, embeddings, max_steps: int = 100, temperature: float = 0.7, top_k: int = 0,
             top_p: float = 0.9, eos_token: int = None, decode: bool = True,
             stop_on_eos: bool = True, seed: int = None, eos_check_every: int = None,
             lengths=None) -> Union[List[str], torch.Tensor]:
    """reference sampling.py:43-121.  Token selection (argmax, or top-k / the reference's top-p rule / softmax /
    multinomial) and the ``(next_token == eos).all()`` test run on the device inside the captured token step; the host
    reads the recorded "first all-eos step" every ``eos_check_every`` steps (default 8, MAGMA_EOS_CHECK_EVERY) instead of
    synchronising on every token, and cuts the output there -- same result as the reference's per-step break.
    ``seed`` fixes the sampling stream (default: drawn from torch's CPU generator, so torch.manual_seed reproduces a run).

    Ragged batches (prompts of different lengths): ``lengths`` (int [B]) gives the prompt length of every row of the
    right-padded ``embeddings`` (B, S_max, d); ``embeddings`` may also be a list of (1, s_i, d) / (s_i, d) tensors, padded
    here.  Row b of the output is then image_token x len_b, the generated tokens, eos up to the width S_max + n (n = steps
    run).  Needs the HIP engine (an LM object without device token selection raises)."""
    eos_token = eos_token or model.eos_token
    was_training = model.training
    if isinstance(embeddings, (list, tuple)):
        embeddings, derived = pad_ragged(embeddings)
        if lengths is not None and not torch.equal(torch.as_tensor(lengths).cpu().to(torch.int64).view(-1), derived):
            raise ValueError(f"lengths {list(lengths)} do not match the per-sample embeddings ({derived.tolist()})")
        lengths = derived
    b, s, _ = embeddings.shape
    dev = embeddings.device
    # the HIP engine selects the token itself; any other LM object gets the reference's call (sampling.py:81-93)
    on_device = getattr(model.lm, "device_token_selection", False)
    if lengths is not None:
        if not on_device:
            raise ValueError("generate(lengths=...) needs the HIP engine's LM (per-row KV positions): this LM object has no "
                             "device token selection and would attend over the padding")
        from .engine import LMEngine
        lengths = LMEngine.check_lengths(lengths, b, s)
    model.eval()
    out = torch.full((b, s + max_steps), eos_token, dtype=torch.long, device=dev)
    out[:, :s] = model.image_token
    n = s
    past = None
    greedy = temperature == 0.0
    mode = None if greedy else (float(temperature), int(top_k), float(top_p))
    if seed is None and not greedy:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    every = eos_check_every or int(os.environ.get("MAGMA_EOS_CHECK_EVERY", "8"))
    first_kw = dict(sampling=mode, eos_token=eos_token, seed=seed) if on_device else {}
    if lengths is not None:
        first_kw["lengths"] = lengths
    step_kw = dict(sampling=mode) if on_device else {}
    for i in range(max_steps):
        if i == 0:
            outputs = model.lm(inputs_embeds=embeddings, use_cache=True, past_key_values=None, cache_hint=max_steps,
                               reuse_cache=True, **first_kw)
        elif on_device:      # the token selected by the previous step is fed back on the device: nothing crosses the host
            outputs = model.lm(input_ids=None, use_cache=True, past_key_values=past, feed_back=True, **step_kw)
        else:
            outputs = model.lm(input_ids=out[:, n - 1:n], use_cache=True, past_key_values=past, **step_kw)
        past = outputs.past_key_values
        if on_device:
            n += 1
            if stop_on_eos and eos_token is not None and ((i + 1) % every == 0 or i + 1 == max_steps):
                first = int(outputs.eos_state[1])            # one host sync per `every` steps
                if first >= 0:
                    n = s + first + 1                        # tokens after the first all-eos step are dropped again
                    break
            continue
        logits = outputs.logits[:, -1, :].float()            # any other LM object: the reference's host-side arithmetic
        if greedy:
            next_token = outputs.next_token.unsqueeze(1) if outputs.get("next_token") is not None else \
                torch.argmax(logits, dim=-1, keepdim=True)
        else:
            if top_k > 0:
                logits = top_k_filter(logits, k=top_k)
            if top_p > 0:
                logits = top_p_filter(logits, threshold=top_p)
            probs = F.softmax(logits / temperature, dim=-1)
            next_token = torch.multinomial(probs, num_samples=1)
        out[:, n:n + 1] = next_token
        n += 1
        if stop_on_eos and eos_token is not None and bool((next_token == eos_token).all()):
            break
    if on_device and lengths is not None:     # ragged: row b's tokens follow its own prompt, eos after them
        n_gen = n - s                         # (no host sync: the next call's launches queue behind this one)
        lens = lengths.to(dev, non_blocking=True)[:, None]
        out.fill_(eos_token)
        out.masked_fill_(torch.arange(s + max_steps, device=dev)[None, :] < lens, model.image_token)
        out.scatter_(1, lens + torch.arange(n_gen, device=dev)[None, :], past.history[:, :n_gen])
        model.lm.engine.check_decode(past)
    elif on_device:          # one copy of the token history the bookkeeping kernel kept
        out[:, s:n] = past.history[:, : n - s]
        model.lm.engine.check_decode(past)
    out = out[:, :n]
    if decode:
        out = [model.tokenizer.decode(remove_tokens_after_eos(row, eos_token, model.image_token)) for row in out]
    model.train(was_training)
    return out
