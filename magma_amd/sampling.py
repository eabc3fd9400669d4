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
import contextlib
import math
import os
from typing import Callable, List, NamedTuple, Optional, Tuple, Union

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


SAMPLERS = ("reference", "transformers")
_FIX = float(2 ** 40)


def check_sampler_args(sampler="reference", min_p=0.0, top_p=0.9):
    """ValueError for sampler arguments generate() does not take.  Returns None for the reference's sampler (the default: its
    top-k keeps exactly k, its top-p is ``top_p_filter``), else dict(min_p float): transformers' sampler -- ``top_k_filter_ties``,
    ``nucleus_filter``, ``min_p_filter`` at the temperature, in that order."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0.0 <= min_p <= 1.0:
        raise ValueError(f"min_p must be a number in [0, 1], got {min_p!r}")
    if sampler == "reference":
        if min_p > 0:
            raise ValueError('min_p needs sampler="transformers": the reference\'s sampler has no min-p rule')
        return None
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0.0 <= top_p <= 1.0:
        raise ValueError(f'sampler="transformers" takes top_p in [0, 1] (0 and 1: off), got {top_p!r}')
    return dict(min_p=float(min_p))


def top_k_filter_ties(logits, k):
    """transformers' TopKLogitsWarper: every logit below the k-th largest of its row becomes -inf -- every tie AT the k-th value
    stays (``top_k_filter`` keeps exactly k).  k == 0 and k >= V: off."""
    if k <= 0 or k >= logits.shape[-1]:
        return logits.clone()
    kth = torch.topk(logits, k).values[..., -1:]
    return logits.masked_fill(logits < kth, float("-inf"))


def nucleus_filter(logits, top_p, temperature: float = 1.0):
    """transformers' TopPLogitsWarper (min_tokens_to_keep = 1) without a sort, the statement csrc/sampling.hip shares (DESIGN.md
    "transformers' sampler").  ``logits`` (R, V) are the RAW logits of the survivors so far (-inf: gone); the probabilities are
    those at ``temperature``.  With q_i = floor(exp((x_i - max) / T) / Z * 2^40 + 0.5) (float64), total = sum q_i and
    c = (uint64)((double)(float)(1 - top_p) * 2^40), token i stays iff the mass ranked before it in descending order is below
    max(total - c, 1); of equal logits at the boundary the j-th by index has preceding mass above + j * q and the first ones stay.
    Applies for 0 < top_p < 1 (0 keeps this project's meaning "off").  Returns a new tensor."""
    bound = float(torch.tensor(1.0 - float(top_p), dtype=torch.float64).to(torch.float32))
    if not (float(top_p) > 0.0 and bound > 0.0):
        return logits.clone()
    c = int(bound * _FIX)
    x = logits.double()
    T = float(torch.tensor(float(temperature), dtype=torch.float32))          # the launch argument is fp32
    w = torch.exp((x - x.max(-1, keepdim=True).values) / T)
    q = torch.floor(w / w.sum(-1, keepdim=True) * _FIX + 0.5).to(torch.int64)
    out = logits.clone()
    for r in range(x.shape[0]):
        limit = max(int(q[r].sum()) - c, 1)
        vals, inv = torch.unique(x[r], sorted=True, return_inverse=True)      # ascending distinct values
        n = torch.bincount(inv, minlength=vals.numel())
        mass = torch.zeros(vals.numel(), dtype=torch.int64).scatter_add_(0, inv, q[r])
        above = mass.flip(0).cumsum(0).flip(0) - mass                       # mass of the strictly larger values
        q_eq = mass // n.clamp(min=1)
        # ties of one value: j stays iff above + j * q_eq < limit  ->  m = ceil((limit - above) / q_eq) of them, at most n
        room = limit - above
        m = torch.where(room <= 0, torch.zeros_like(n),
                        torch.where(q_eq > 0, torch.minimum(n, (room + q_eq - 1) // q_eq.clamp(min=1)), n))
        order = torch.argsort(inv, stable=True)                              # by value, then by index
        rank = torch.empty_like(order)
        start = torch.cumsum(n, 0) - n
        rank[order] = torch.arange(order.numel()) - start[inv[order]]        # index rank among the ties of the value
        out[r] = out[r].masked_fill(rank >= m[inv], float("-inf"))
    return out


def min_p_filter(logits, min_p, temperature: float = 1.0):
    """transformers' MinPLogitsWarper (min_tokens_to_keep = 1): a token goes iff p_i < min_p * p_max at ``temperature``, i.e.
    exp((x_i - max) / T) < min_p in float64 -- a ratio that renormalising the survivors of top-k / top-p does not change.
    ``logits`` (R, V) raw.  min_p == 0: off.  A maximum is never dropped.  Returns a new tensor."""
    if not float(min_p) > 0.0:
        return logits.clone()
    x = logits.double()
    T = float(torch.tensor(float(temperature), dtype=torch.float32))
    d = x - x.max(-1, keepdim=True).values
    return logits.masked_fill((torch.exp(d / T) < float(min_p)) & (d < 0), float("-inf"))


def warp_filter(logits, temperature, top_k=0, top_p=0.0, min_p=0.0):
    """The chain of transformers' sampler on RAW logits (R, V): top-k with ties, nucleus top-p and min-p at ``temperature``.
    Returns the raw logits with -inf where a rule dropped the token; the draw is softmax(that / temperature)."""
    x = top_k_filter_ties(logits, int(top_k))
    x = nucleus_filter(x, top_p, temperature)
    return min_p_filter(x, min_p, temperature)


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


def is_embed_batch(x) -> bool:
    """embed_batch's (embeddings (B, S, d), lengths [B] integers) -- as opposed to a tuple of per-sample embeddings."""
    if not (isinstance(x, tuple) and len(x) == 2 and torch.is_tensor(x[0]) and x[0].ndim == 3):
        return False
    lens = torch.as_tensor(x[1]) if not torch.is_tensor(x[1]) else x[1]
    return lens.ndim == 1 and not lens.is_floating_point() and not lens.is_complex() and lens.dtype != torch.bool


def prompt_batch(embeddings, lengths=None, *, check: bool = True, name: str = "lengths", per_row: bool = True):
    """The prompt forms every entry point takes -- a (B, S, d) tensor with optional ``lengths``, a list of per-sample tensors,
    embed_batch's (embeddings, lengths) -- as (right-padded (B, S, d) tensor, lengths or None).  A list is padded and gives its
    own lengths; ``lengths`` passed beside it must agree.  ``check``: the lengths come back as LMEngine.check_lengths' host
    int64 [B] tensor (1 <= len_b <= S) -- refused when the LM keeps no KV position ``per_row`` (only the HIP engine does).
    ``name``: what the error calls the lengths."""
    if is_embed_batch(embeddings):
        embeddings, lengths = embeddings
    if isinstance(embeddings, (list, tuple)):
        embeddings, derived = pad_ragged(embeddings)
        if lengths is not None and not torch.equal(torch.as_tensor(lengths).cpu().to(torch.int64).view(-1), derived):
            raise ValueError(f"{name} {list(lengths)} do not match the per-sample embeddings ({derived.tolist()})")
        lengths = derived
    if check and lengths is not None:
        if not per_row:
            raise ValueError("generate(lengths=...) needs the HIP engine's LM (per-row KV positions): this LM object has no "
                             "device token selection and would attend over the padding")
        from .engine import LMEngine
        lengths = LMEngine.check_lengths(lengths, embeddings.shape[0], embeddings.shape[1])
    return embeddings, lengths


MAX_NGRAM, MAX_SUPPRESS = 16, 1024


def check_processor_args(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, vocab: int = None):
    """ValueError for values the logits processors do not take.  Returns None when all four are neutral (nothing is applied,
    nothing is launched), else dict(repetition_penalty float, no_repeat_ngram_size int, min_new_tokens int, suppress_tokens
    tuple of ints).  ``vocab``: the number of logits V, when known -- suppress ids must lie in [0, V)."""
    p = repetition_penalty
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not p > 0 or p == float("inf"):
        raise ValueError(f"repetition_penalty must be a number > 0, got {p!r}")
    n = no_repeat_ngram_size
    if isinstance(n, bool) or not isinstance(n, int) or n < 0 or n > MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size must be an integer in [0, {MAX_NGRAM}], got {n!r}")
    m = min_new_tokens
    if isinstance(m, bool) or not isinstance(m, int) or m < 0:
        raise ValueError(f"min_new_tokens must be an integer >= 0, got {m!r}")
    if torch.is_tensor(suppress_tokens):
        suppress_tokens = suppress_tokens.tolist()
    ids = tuple(suppress_tokens) if suppress_tokens is not None else ()
    if len(ids) > MAX_SUPPRESS:
        raise ValueError(f"suppress_tokens takes at most {MAX_SUPPRESS} ids, got {len(ids)}")
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
            raise ValueError(f"suppress_tokens must be token ids in [0, {'V' if vocab is None else vocab}), got {t!r}")
    if float(p) == 1.0 and n == 0 and m == 0 and not ids:
        return None
    return dict(repetition_penalty=float(p), no_repeat_ngram_size=n, min_new_tokens=m, suppress_tokens=ids)


def process_logits(scores, history, step: int, *, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                   min_new_tokens: int = 0, eos_token: int = None, suppress_tokens=()):
    """The logits processors, host statement (the device kernel is csrc/sampling.hip, logits_process_kernel): the rules of
    transformers' RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor and
    SuppressTokensLogitsProcessor in the order GenerationMixin._get_logits_processor chains them, with the prompt passed as
    embeddings: the processors' ``input_ids`` are the generated tokens only.

    ``scores`` (R, V) fp32; row r has generated ``history[r, :step]`` (``history`` (R, >= step) int64).  Returns a new tensor.
      repetition penalty p   every distinct token t of the row's history, once: x[t] = x[t] * p if x[t] < 0 else x[t] / p
      no-repeat n-gram n     if step >= n: every window start w in [0, step - n] whose n - 1 tokens equal the last n - 1 tokens
                             bans history[w + n - 1] (-inf); n = 1 bans every generated token
      min new tokens         step < min_new_tokens: x[eos] = -inf (``eos_token``: one id, or a sequence of ids -- every one)
      suppress               x[t] = -inf for every listed t
    Greedy and sampled selection apply this to the raw logits (before temperature / top-k / top-p), beam search to
    log_softmax(logits) without renormalising, as transformers does."""
    x = scores.clone()
    R, V = x.shape
    hist = history[:, :step].to(torch.int64)
    p = float(repetition_penalty)
    if p != 1.0 and step > 0:
        got = torch.gather(x, 1, hist)
        x = x.scatter(1, hist, torch.where(got < 0, got * p, got / p))
    n = int(no_repeat_ngram_size)
    if n > 0 and step >= n:
        prefix = hist[:, step + 1 - n:]
        windows = hist.unfold(1, n, 1)                                          # (R, step - n + 1, n)
        match = (windows[..., :-1] == prefix[:, None, :]).all(-1)
        banned = torch.zeros(R, V + 1, dtype=torch.bool)
        banned.scatter_(1, torch.where(match, windows[..., -1], V), True)       # non-matching windows land in a spare column
        x = x.masked_fill(banned[:, :V], float("-inf"))
    if step < int(min_new_tokens) and eos_token is not None:
        if isinstance(eos_token, (list, tuple)):
            x[:, torch.tensor([int(t) for t in eos_token], dtype=torch.int64)] = float("-inf")
        else:
            x[:, int(eos_token)] = float("-inf")
    ids = list(suppress_tokens) if suppress_tokens is not None else []
    if ids:
        x[:, torch.tensor(ids, dtype=torch.int64)] = float("-inf")
    return x


MAX_TRIE_LEN, MAX_TRIE_SEQS, MAX_TRIE_NODES = 64, 65536, 2 ** 20


class TrieRows(NamedTuple):
    """A trie's non-root nodes in depth-first preorder (TokenTrie.rows; DESIGN.md "Ranking choices"): int32 tensors."""
    token: torch.Tensor         # [N]: the edge into node i
    parent: torch.Tensor        # [N]: the row of its parent, -1 for a child of the root
    off: torch.Tensor           # [N]: depth - 1; the token is fed at position p + off[i]
    sub: torch.Tensor           # [N]: one past the last row of node i's subtree: j is i or an ancestor of i iff j <= i < sub[j]
    terminal: torch.Tensor      # [N]: a listed sequence ends here
    leaf_of: torch.Tensor       # [C]: the row of listed sequence c


def pad_trie_rows(rows) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(token, off, sub) int32 [B, T] of a batch of TrieRows (None: a row without a tree), right-padded to T = the most nodes
    of a row: a padding row carries token 0, off 0 and sub[t] = t + 1 -- it sees the prompt and itself, nobody sees it."""
    T = max([1] + [r.token.numel() for r in rows if r is not None])
    token, off = torch.zeros(len(rows), T, dtype=torch.int32), torch.zeros(len(rows), T, dtype=torch.int32)
    sub = (torch.arange(T, dtype=torch.int32) + 1).repeat(len(rows), 1)
    for b, r in enumerate(rows):
        if r is not None:
            n = r.token.numel()
            token[b, :n], off[b, :n], sub[b, :n] = r.token, r.off, r.sub
    return token, off, sub


class TokenTrie:
    """An immutable trie over token-id sequences: the closed set of answers ``generate(constraint=...)`` keeps a row inside
    (DESIGN.md "Constrained decoding").  ``sequences``: at most 65 536 entries, each 1 to 64 ids >= 0 (a list, a tuple, a tensor)
    or a ``str`` that ``encode`` turns into ids (no ``encode``: a ``str`` raises); at most 2^20 nodes.  Duplicates collapse; one
    sequence may be a prefix of another (its node is terminal AND has edges).  Nodes are numbered breadth first from the root 0,
    so a node's edges are consecutive; within a node they ascend by token."""
    __slots__ = ("sequences", "_index", "_kids", "first", "terminal", "parent", "in_token", "edge_token", "edge_child", "_tokens",
                 "_flat")

    def __init__(self, sequences, encode: Callable = None):
        if isinstance(sequences, str) or not isinstance(sequences, (list, tuple)):
            raise ValueError("a TokenTrie takes a list of token-id sequences or strings")
        if not 1 <= len(sequences) <= MAX_TRIE_SEQS:
            raise ValueError(f"a TokenTrie takes 1 to {MAX_TRIE_SEQS} sequences, got {len(sequences)}")
        seqs = []
        for q in sequences:
            if isinstance(q, str):
                if encode is None:
                    raise ValueError(f"the sequence {q!r} is text and there is no tokenizer to encode it")
                q = encode(q)
            if torch.is_tensor(q):
                q = q.tolist()
            if not isinstance(q, (list, tuple)) or not 1 <= len(q) <= MAX_TRIE_LEN:
                raise ValueError(f"a sequence is 1 to {MAX_TRIE_LEN} token ids, got {q!r}")
            for t in q:
                if isinstance(t, bool) or not isinstance(t, int) or t < 0 or t >= 2 ** 31:
                    raise ValueError(f"a sequence holds token ids >= 0, got {t!r}")
            seqs.append(tuple(q))
        kids, term = [{}], [False]
        for q in seqs:
            n = 0
            for t in q:
                c = kids[n].get(t)
                if c is None:
                    c = kids[n][t] = len(kids)
                    kids.append({})
                    term.append(False)
                n = c
            term[n] = True
        if len(kids) > MAX_TRIE_NODES:
            raise ValueError(f"a TokenTrie holds at most {MAX_TRIE_NODES} nodes, these sequences need {len(kids)}")
        order, new = [0], {0: 0}
        for n in order:                     # breadth first, edges ascending
            for t in sorted(kids[n]):
                new[kids[n][t]] = len(order)
                order.append(kids[n][t])
        N = len(order)
        first, parent, in_token, etok, echild = [0], [-1] * N, [-1] * N, [], []
        for i, n in enumerate(order):
            for t in sorted(kids[n]):
                c = new[kids[n][t]]
                etok.append(t)
                echild.append(c)
                parent[c], in_token[c] = i, t
            first.append(len(etok))
        index = {}
        for i, q in enumerate(seqs):
            index.setdefault(q, i)
        set_ = object.__setattr__
        set_(self, "sequences", tuple(seqs))
        set_(self, "_index", index)
        set_(self, "_kids", tuple({t: new[c] for t, c in kids[n].items()} for n in order))
        set_(self, "first", tuple(first))
        set_(self, "terminal", tuple(int(term[n]) for n in order))
        set_(self, "parent", tuple(parent))
        set_(self, "in_token", tuple(in_token))
        set_(self, "edge_token", tuple(etok))
        set_(self, "edge_child", tuple(echild))
        set_(self, "_tokens", frozenset(etok))
        set_(self, "_flat", torch.tensor([N, len(etok)] + first + list(self.terminal) + parent + in_token + etok + echild,
                                         dtype=torch.int32))

    def __setattr__(self, name, value):
        raise AttributeError("a TokenTrie is immutable")

    @property
    def n_nodes(self) -> int:
        return len(self.terminal)

    @property
    def n_edges(self) -> int:
        return len(self.edge_token)

    def tokens(self) -> frozenset:
        """Every token id of every sequence."""
        return self._tokens

    def min_len(self) -> int:
        return min(len(q) for q in self.sequences)

    def max_len(self) -> int:
        return max(len(q) for q in self.sequences)

    def index(self, tokens) -> int:
        """The position of the sequence ``tokens`` in the constructor's list (of duplicates: the first), or -1."""
        if torch.is_tensor(tokens):
            tokens = tokens.tolist()
        return self._index.get(tuple(int(t) for t in tokens), -1)

    def node(self, prefix):
        """The node the walk of ``prefix`` from the root ends at, or None when it leaves the trie."""
        n = 0
        for t in prefix:
            n = self._kids[n].get(int(t))
            if n is None:
                return None
        return n

    def allowed(self, prefix, eos_ids) -> List[int]:
        """The host rule: after the generated tokens ``prefix`` -- at node n: the tokens of n's edges, plus every eos id if n is
        terminal; off the trie (a token that is no edge, an eos taken at a terminal node and the padding behind it included):
        the eos ids alone.  Never empty: a leaf is terminal.  Usable as transformers' ``prefix_allowed_tokens_fn`` body."""
        if torch.is_tensor(prefix):
            prefix = prefix.tolist()
        eos = [int(t) for t in eos_ids]
        n = self.node(prefix)
        if n is None:
            return eos
        return list(self.edge_token[self.first[n]: self.first[n + 1]]) + (eos if self.terminal[n] else [])

    def flat(self) -> torch.Tensor:
        """The int32 table the device reads (layout: include/magma_hip.h, mg_logits_process_constrained_f32): {n_nodes, n_edges},
        first[n_nodes + 1], terminal[n_nodes], parent[n_nodes], in_token[n_nodes], edge_token[n_edges], edge_child[n_edges]."""
        return self._flat.clone()

    def rows(self, select=None) -> "TrieRows":
        """The non-root nodes in depth-first preorder (edges ascending), the table ``rank`` feeds one forward with (DESIGN.md
        "Ranking choices"): ``TrieRows`` of int32 tensors -- token[i] the edge into node i, parent[i] the row of its parent (-1: a
        child of the root), off[i] = depth - 1 (the token is fed at position p + off[i]), sub[i] one past the last row of node
        i's subtree, terminal[i], and leaf_of[c] the row of listed sequence c (duplicates share a row).  In preorder "j is i or an
        ancestor of i" is j <= i < sub[j].  ``select``: positions of the constructor's list -- the rows of the trie of those
        sequences only (leaf_of in that order); preorder keeps a node's row number when later sequences are left out."""
        seqs = self.sequences if select is None else [self.sequences[c] for c in select]
        order = sorted(set(seqs))               # lexicographic over the distinct sequences = preorder, edges ascending
        token, parent, off, terminal, row_at = [], [], [], [], {}
        path = []                               # rows of the current root-to-node path
        prev = ()
        for q in order:
            keep = 0
            while keep < min(len(prev), len(q)) and prev[keep] == q[keep]:
                keep += 1
            del path[keep:]
            for d in range(keep, len(q)):
                parent.append(path[-1] if path else -1)
                path.append(len(token))
                token.append(q[d])
                off.append(d)
                terminal.append(0)
            terminal[path[-1]] = 1
            row_at[q] = path[-1]
            prev = q
        n = len(token)
        sub = [i + 1 for i in range(n)]
        for i in range(n - 1, -1, -1):          # a parent precedes its children: fold the subtree ends upwards
            if parent[i] >= 0:
                sub[parent[i]] = max(sub[parent[i]], sub[i])
        i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
        return TrieRows(i32(token), i32(parent), i32(off), i32(sub), i32(terminal), i32([row_at[q] for q in seqs]))

    @staticmethod
    def from_flat(table) -> List[tuple]:
        """The sequences a one-trie table holds, in breadth-first order of their last node (flat()'s inverse up to order)."""
        t = torch.as_tensor(table).tolist()
        n, e = t[0], t[1]
        terminal, parent, in_token = t[3 + n: 3 + 2 * n], t[3 + 2 * n: 3 + 3 * n], t[3 + 3 * n: 3 + 4 * n]
        assert len(t) == 3 + 4 * n + 2 * e
        out = []
        for i in range(n):
            if terminal[i]:
                q, j = [], i
                while parent[j] >= 0:
                    q.append(in_token[j])
                    j = parent[j]
                out.append(tuple(reversed(q)))
        return out


def trie_forest(tries) -> Tuple[torch.Tensor, torch.Tensor]:
    """(table int32, roots int32 [len(tries)]): the distinct tries of ``tries`` side by side in one table of TokenTrie.flat()'s
    layout -- node and edge numbers shifted by what stands before them -- and, per entry, the node that is its root."""
    distinct, at = [], {}
    for t in tries:
        if id(t) not in at:
            at[id(t)] = len(distinct)
            distinct.append(t)
    if len(distinct) == 1:      # the table made once, when the trie was built
        return distinct[0]._flat, torch.zeros(len(tries), dtype=torch.int32)
    first, terminal, parent, in_token, etok, echild, root_of = [], [], [], [], [], [], []
    n_off = e_off = 0
    for t in distinct:
        root_of.append(n_off)
        first += [f + e_off for f in t.first[:-1]]
        terminal += t.terminal
        parent += [p + n_off if p >= 0 else -1 for p in t.parent]
        in_token += t.in_token
        etok += t.edge_token
        echild += [c + n_off for c in t.edge_child]
        n_off, e_off = n_off + t.n_nodes, e_off + t.n_edges
    table = torch.tensor([n_off, e_off] + first + [e_off] + terminal + parent + in_token + etok + echild, dtype=torch.int32)
    return table, torch.tensor([root_of[at[id(t)]] for t in tries], dtype=torch.int32)


def check_constraint_args(constraint, batch: int = None, encode: Callable = None, vocab: int = None, eos_ids=(), proc: dict = None):
    """ValueError for a ``constraint`` generate() does not take.  Returns None (``constraint`` None: today's call) or a list of
    TokenTrie, one per row (one object repeated when the rows share it; a list of length 1 when ``batch`` is None).  Forms: a
    TokenTrie; a list of sequences (id lists / tensors / ``str`` for ``encode``); a list of ``batch`` of either, one per row.
    Refused, because they could leave a row without any token: ``no_repeat_ngram_size`` > 0, ``min_new_tokens`` above the
    shortest sequence, ``suppress_tokens`` that meet the trie's tokens or the eos ids (``proc``: check_processor_args' dict),
    and a trie id >= ``vocab``."""
    if constraint is None:
        return None

    def is_seq(q):
        return isinstance(q, str) or torch.is_tensor(q) or (isinstance(q, (list, tuple)) and len(q) > 0 and
                                                            all(isinstance(t, int) and not isinstance(t, bool) for t in q))

    def one(c):
        return c if isinstance(c, TokenTrie) else TokenTrie(c, encode)

    if isinstance(constraint, TokenTrie):
        tries = [constraint] * (batch or 1)
    elif isinstance(constraint, (list, tuple)) and len(constraint) > 0 and all(is_seq(q) for q in constraint):
        tries = [TokenTrie(constraint, encode)] * (batch or 1)
    elif isinstance(constraint, (list, tuple)) and len(constraint) > 0:
        if batch is not None and len(constraint) != batch:
            raise ValueError(f"a per-row constraint needs one entry per row: {len(constraint)} entries for {batch} rows")
        tries = [one(c) for c in constraint]
    else:
        raise ValueError("constraint must be a TokenTrie, a list of sequences, or a list of one of either per row")
    distinct = list({id(t): t for t in tries}.values())
    toks = frozenset().union(*(t.tokens() for t in distinct))
    if vocab is not None and max(toks) >= vocab:
        raise ValueError(f"the constraint holds token ids outside [0, {vocab}): {sorted(t for t in toks if t >= vocab)[:8]}")
    if proc is not None:
        if proc["no_repeat_ngram_size"] > 0:
            raise ValueError("no_repeat_ngram_size is not combined with a constraint: it could ban every token the trie allows")
        shortest = min(t.min_len() for t in distinct)
        if proc["min_new_tokens"] > shortest:
            raise ValueError(f"min_new_tokens = {proc['min_new_tokens']} exceeds the constraint's shortest sequence ({shortest} "
                             "tokens): at its end only eos is allowed, and eos would be banned")
        hit = sorted(set(proc["suppress_tokens"]) & (toks | {int(t) for t in eos_ids}))
        if hit:
            raise ValueError(f"suppress_tokens meets the constraint's tokens or the eos ids ({hit[:8]}): a row could be left "
                             "without any token")
    return tries


def constrain_logits(scores, history, step: int, tries, eos_ids):
    """The trie constraint, host statement (the device kernel is csrc/sampling.hip, logits_process_constrained_kernel): the rule
    of transformers' ``PrefixConstrainedLogitsProcessor(lambda b, ids: tries[b].allowed(ids.tolist(), eos_ids), 1)`` with the
    prompt passed as embeddings -- ``input_ids`` are the generated tokens only.

    ``scores`` (R, V) fp32; row r has generated ``history[r, :step]``; ``tries``: one TokenTrie for every row, or a list of R.
    Row r keeps the columns ``tries[r].allowed(history[r, :step], eos_ids)`` (ids outside [0, V) are skipped); every other
    column becomes -inf.  Returns a new tensor.  It follows the repetition penalty in the chain; the other rules only write
    -inf, so their order among themselves and with this one does not matter."""
    R, V = scores.shape
    if isinstance(tries, TokenTrie):
        tries = [tries] * R
    if len(tries) != R:
        raise ValueError(f"{len(tries)} tries for {R} rows")
    hist = torch.as_tensor(history)[:, :step].to(torch.int64).cpu().tolist()
    keep = torch.zeros(R, V, dtype=torch.bool)
    for r in range(R):
        ids = [t for t in tries[r].allowed(hist[r], eos_ids) if 0 <= t < V]
        if ids:
            keep[r, torch.tensor(ids, dtype=torch.int64)] = True
    return scores.masked_fill(~keep.to(scores.device), float("-inf"))


def check_guidance_values(guidance_scale=1.0, guidance_min_p=0.0):
    """ValueError for a guidance scale that is not a finite number >= 0, or a guidance_min_p outside [0, 1]."""
    g = guidance_scale
    if isinstance(g, bool) or not isinstance(g, (int, float)) or not 0.0 <= g < float("inf"):
        raise ValueError(f"guidance_scale must be a finite number >= 0 (1.0 = off), got {g!r}")
    m = guidance_min_p
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not 0.0 <= m <= 1.0:
        raise ValueError(f"guidance_min_p must be a number in [0, 1] (0 = off), got {m!r}")


def check_guidance_args(guidance_scale=1.0, negative_embeddings=None, negative_lengths=None, guidance_min_p=0.0, batch: int = None,
                        hidden: int = None):
    """ValueError for guidance arguments generate() does not take.  Returns None at the defaults (the call as it was) or
    dict(scale float, min_p float, embeddings (B, S', d) tensor, lengths int64 [B] on the host or None).
    ``negative_embeddings`` takes what ``embeddings`` takes: a (B, S', d) tensor, a (1, S', d) tensor (broadcast to every row), a
    list of per-row tensors, or embed_batch's (embeddings, lengths); ``negative_lengths`` belongs to the tensor forms.  Refused: a
    scale != 1 without a negative prompt, a negative prompt or ``guidance_min_p`` > 0 with scale == 1, and -- ``batch`` / ``hidden``
    given -- a row count other than 1 or ``batch`` or another hidden size."""
    check_guidance_values(guidance_scale, guidance_min_p)
    scale, min_p = float(guidance_scale), float(guidance_min_p)
    if scale == 1.0:
        if negative_embeddings is not None or negative_lengths is not None:
            raise ValueError("a negative prompt has no effect at guidance_scale = 1.0: pass a scale != 1 or leave it out")
        if min_p > 0.0:
            raise ValueError("guidance_min_p has no effect at guidance_scale = 1.0: it is the cut of the guidance rule")
        return None
    if negative_embeddings is None:
        raise ValueError(f"guidance_scale = {scale} needs negative_embeddings (the negative / unconditional prompt)")
    neg, lens = negative_embeddings, negative_lengths
    if is_embed_batch(neg) and lens is not None:
        raise ValueError("negative_embeddings already carries its lengths")
    neg, lens = prompt_batch(neg, lens, check=False, name="negative_lengths")       # (its own range check follows)
    if not torch.is_tensor(neg) or neg.ndim != 3 or neg.shape[1] < 1:
        raise ValueError("negative_embeddings must be a (B, S', d) or (1, S', d) tensor, a list of per-row tensors or "
                         "embed_batch's (embeddings, lengths)")
    if lens is not None:
        lens = torch.as_tensor(lens).detach().cpu()
        if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool or lens.ndim != 1 or \
                lens.shape[0] != neg.shape[0] or int(lens.min()) < 1 or int(lens.max()) > neg.shape[1]:
            raise ValueError(f"negative_lengths must be {neg.shape[0]} integers in [1, {neg.shape[1]}], got {lens.tolist()}")
        lens = lens.to(torch.int64)
    if hidden is not None and neg.shape[2] != hidden:
        raise ValueError(f"negative_embeddings has hidden size {neg.shape[2]}, the prompt {hidden}")
    if batch is not None:
        if neg.shape[0] not in (1, batch):
            raise ValueError(f"negative_embeddings has {neg.shape[0]} rows, the prompt {batch} (1 row is broadcast)")
        if neg.shape[0] != batch:
            neg = neg.expand(batch, -1, -1)
            lens = None if lens is None else lens.expand(batch).clone()
    return dict(scale=scale, min_p=min_p, embeddings=neg, lengths=lens)


def guide_logits(cond, uncond, guidance_scale, guidance_min_p=0.0):
    """Classifier-free guidance, host statement (the device kernel is csrc/sampling.hip, logits_guidance_kernel) in float64 from
    fp32 inputs: ``cond`` / ``uncond`` (R, V), the logits of the same step under the prompt and under the negative prompt.
        c = log_softmax(cond), u = log_softmax(uncond)
        out = u + guidance_scale * (c - u)
        out[i] = -inf  where  cond[i] - max(cond) < log(guidance_min_p)        (guidance_min_p > 0 only)
    The first two lines are transformers' ``UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__``; the third is the
    plausibility cut of contrastive decoding (Li et al. 2023): without it a large scale promotes tokens that are impossible under
    the conditional model merely because the negative model finds them even less likely.  The cut compares the fp32 difference
    of the RAW conditional logits with the fp32 rounding of the float64 log -- no logsumexp takes part, so host and device keep
    exactly the same set; the row maximum always stays, ties at the bound stay.  ``guidance_scale`` finite and >= 0 (1: c
    itself), ``guidance_min_p`` in [0, 1] (0: off).  A conditional -inf stays -inf (whatever the scale, 0 included).  The
    unconditional logits must be finite (ValueError): u = -inf under c > -inf would give +inf.  Returns float64 (R, V)."""
    check_guidance_values(guidance_scale, guidance_min_p)
    c32 = torch.as_tensor(cond).detach().cpu().to(torch.float32)
    u32 = torch.as_tensor(uncond).detach().cpu().to(torch.float32)
    if c32.ndim != 2 or c32.shape != u32.shape:
        raise ValueError(f"cond and uncond must be (R, V) alike, got {tuple(c32.shape)} / {tuple(u32.shape)}")
    if not bool(torch.isfinite(u32).all()):
        raise ValueError("the unconditional logits must be finite")
    c, u = F.log_softmax(c32.double(), dim=-1), F.log_softmax(u32.double(), dim=-1)
    out = u + float(guidance_scale) * (c - u)
    out = out.masked_fill(c32 == float("-inf"), float("-inf"))
    if float(guidance_min_p) > 0.0:
        bound = torch.tensor(float(guidance_min_p), dtype=torch.float64).log().to(torch.float32)
        out = out.masked_fill((c32 - c32.max(-1, keepdim=True).values) < bound, float("-inf"))
    return out


MAX_EOS_IDS, MAX_STOP_SEQS, MAX_STOP_LEN = 8, 16, 16
REASON_NONE, REASON_EOS, REASON_STOP = 0, 1, 2
REASON_LENGTH = 3       # a slot session's row reached its own max_new_tokens (the device's MG_STOP_LEN >> 8)
REASON_NAMES = {REASON_NONE: "length", REASON_EOS: "eos", REASON_STOP: "stop", REASON_LENGTH: "length"}


class Finish(NamedTuple):
    """How every row of a per-row generate() call ended (``return_finish=True``)."""
    kept: torch.Tensor          # int64 [B]: the generated tokens of the row that count, the finishing token included
    reason: List[str]           # "eos" | "stop" | "length" (the row ran to the end of the call)
    index: List[int]            # which eos id / which stop sequence (-1 for "length")


def check_stop_args(eos_token, stop_sequences=None, stop_per_row=None, vocab: int = None, encode: Callable = None):
    """ValueError for stopping arguments generate() does not take.  Returns None when the call keeps the reference's rule (one
    eos id, the batch ends at the first step at which every row selects it), else dict(eos_ids tuple of 1 to 8 ints,
    stop_seqs tuple of at most 16 tuples of 1 to 16 ints): the per-row rule of ``stop_update``.  ``stop_per_row`` None means
    per-row exactly when ``eos_token`` is a sequence or ``stop_sequences`` is given.  ``vocab``: the number of logits V, when
    known -- every id must lie in [0, V).  ``encode``: turns a ``str`` entry of ``stop_sequences`` into token ids."""
    def ident(t, what):
        if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
            raise ValueError(f"{what} must be token ids in [0, {'V' if vocab is None else vocab}), got {t!r}")
        return t

    if torch.is_tensor(eos_token):
        eos_token = eos_token.tolist()
    listed = isinstance(eos_token, (list, tuple))
    eos_ids = tuple(eos_token) if listed else (eos_token,)
    if not 1 <= len(eos_ids) <= MAX_EOS_IDS:
        raise ValueError(f"eos_token takes 1 to {MAX_EOS_IDS} ids, got {len(eos_ids)}")
    wanted = listed or stop_sequences is not None
    if stop_per_row is not None and not isinstance(stop_per_row, bool):
        raise ValueError(f"stop_per_row must be None, True or False, got {stop_per_row!r}")
    if stop_per_row is False and wanted:
        raise ValueError("stop_per_row=False keeps the reference's rule of one eos id for the whole batch: it takes neither a "
                         "list of eos ids nor stop_sequences")
    if not (wanted or stop_per_row):
        return None                       # today's call: its eos id is taken as it always was
    eos_ids = tuple(ident(t, "eos_token") for t in eos_ids)
    seqs = []
    if stop_sequences is not None:
        if isinstance(stop_sequences, str) or not isinstance(stop_sequences, (list, tuple)):
            raise ValueError("stop_sequences must be a list of token-id sequences or strings")
        if len(stop_sequences) > MAX_STOP_SEQS:
            raise ValueError(f"stop_sequences takes at most {MAX_STOP_SEQS} entries, got {len(stop_sequences)}")
        for q in stop_sequences:
            if isinstance(q, str):
                if encode is None:
                    raise ValueError(f"the stop sequence {q!r} is text and this model has no tokenizer to encode it")
                q = encode(q)
            if torch.is_tensor(q):
                q = q.tolist()
            if not isinstance(q, (list, tuple)) or not 1 <= len(q) <= MAX_STOP_LEN:
                raise ValueError(f"a stop sequence is 1 to {MAX_STOP_LEN} token ids, got {q!r}")
            seqs.append(tuple(ident(t, "stop_sequences") for t in q))
    return dict(eos_ids=eos_ids, stop_seqs=tuple(seqs))


def stop_update(history, step: int, done, eos_ids, stop_seqs=()):
    """The per-row stopping rule, host statement (the device kernel is csrc/sampling.hip, sample_finish_rows_kernel): the row
    test of transformers' ``GenerationMixin._sample`` -- EosTokenCriteria with a list of ids, plus stop sequences over token ids
    -- with the prompt passed as embeddings: only the tokens generated by this call take part.

    ``history`` (R, > step) int64 holds every row's tokens of steps 0 .. step (finished rows: the pad id from the step after
    they finished), ``done`` (R,) bool the rows that finished at an earlier step.  A row that is not done finishes at this step
      eos    if history[r, step] is one of ``eos_ids`` (1 to 8): reason (REASON_EOS, index of the id), tested first;
      stop   if history[r, :step + 1] ends with one of ``stop_seqs`` (at most 16 of 1 to 16 ids; one longer than step + 1
             cannot match): reason (REASON_STOP, lowest matching index).
    Returns (done (R,) bool including this step's rows, reason (R, 2) int64 -- (REASON_NONE, -1) for every row that did not
    finish AT this step).  The caller keeps the finishing token, writes ``eos_ids[0]`` (the pad id) for a done row from the next
    step on, and ends the loop after the first step at which every row is done."""
    hist = torch.as_tensor(history).to(torch.int64).cpu()
    done = torch.as_tensor(done).to(torch.bool).cpu().clone()
    R = hist.shape[0]
    reason = torch.tensor([[REASON_NONE, -1]] * R, dtype=torch.int64).view(R, 2)
    for r in range(R):
        if bool(done[r]):
            continue
        t = int(hist[r, step])
        hit = None
        for i, e in enumerate(eos_ids):
            if t == int(e):
                hit = (REASON_EOS, i)
                break
        if hit is None:
            for j, q in enumerate(stop_seqs):
                n = len(q)
                if 1 <= n <= step + 1 and hist[r, step + 1 - n: step + 1].tolist() == [int(x) for x in q]:
                    hit = (REASON_STOP, j)
                    break
        if hit is not None:
            done[r] = True
            reason[r, 0], reason[r, 1] = hit
    return done, reason


def slot_update(ring, step: int, done, begin, limit, eos_ids, stop_seqs=()):
    """The row test of a slot session, host statement (the device kernel is csrc/sampling.hip, sample_finish_slots_kernel):
    ``stop_update`` with a window, a budget and a ring.  ``ring`` (R, Hc) int64 is the token history read as a ring: the column of
    a step is step % Hc, and it already holds this step's tokens.  ``begin`` (R,) is the column of every row's occupant's first
    token, ``limit`` (R,) its max_new_tokens.  The occupant's own token count is n = (step % Hc - begin) mod Hc + 1.  A row that is
    not done finishes at this step
      eos     as in stop_update, tested first;
      stop    if its last L tokens are one of ``stop_seqs`` AND L <= n: tokens of the slot's previous occupant never take part,
              while a sequence that straddles the ring's wrap does match;
      length  if n >= limit without either: reason (REASON_LENGTH, 0).
    Returns (done, reason) as stop_update does.  With begin = 0 and limit, Hc larger than the run it is stop_update."""
    hist = torch.as_tensor(ring).to(torch.int64).cpu()
    done = torch.as_tensor(done).to(torch.bool).cpu().clone()
    R, Hc = hist.shape
    col = step % Hc
    reason = torch.tensor([[REASON_NONE, -1]] * R, dtype=torch.int64).view(R, 2)
    for r in range(R):
        if bool(done[r]):
            continue
        n = (col - int(begin[r])) % Hc + 1
        t = int(hist[r, col])
        hit = None
        for i, e in enumerate(eos_ids):
            if t == int(e):
                hit = (REASON_EOS, i)
                break
        if hit is None:
            for j, q in enumerate(stop_seqs):
                L = len(q)
                if 1 <= L <= n and [int(hist[r, (col - L + 1 + k) % Hc]) for k in range(L)] == [int(x) for x in q]:
                    hit = (REASON_STOP, j)
                    break
        if hit is None and n >= int(limit[r]):
            hit = (REASON_LENGTH, 0)
        if hit is not None:
            done[r] = True
            reason[r, 0], reason[r, 1] = hit
    return done, reason


def slot_tokens(ring_row, begin: int, step: int, cols: int):
    """The tokens a slot's occupant has generated BEFORE step ``step`` (the device's state[0]) selects, in order, host statement
    of the window the slot kernels read (csrc/sampling.hip, slot_window / HistView): ``ring_row`` is the row of the ring history of
    ``cols`` columns, ``begin`` the column of the occupant's first token (slot_update's).  The newest token stands at column
    (step - 1) % cols, so there are n = ((step - 1) % cols - begin) % cols + 1 of them -- the count slot_update forms at the step
    before --, token i at column (begin + i) % cols: a window that reaches the last column goes on at column 0.  n lies in
    [1, cols]; no column outside the window is read."""
    row = torch.as_tensor(ring_row).to(torch.int64).cpu().view(-1)
    begin, step, cols = int(begin), int(step), int(cols)
    if cols < 1 or row.numel() < cols or not 0 <= begin < cols:
        raise ValueError(f"need a ring row of at least cols = {cols} >= 1 columns and 0 <= begin < cols, got begin = {begin}")
    n = ((step - 1) % cols - begin) % cols + 1
    return row[(begin + torch.arange(n)) % cols].clone()


def finish_from_record(record, n_gen: int) -> Finish:
    """``record`` (B, 2) integers = (step at which the row finished or -1, reason * 256 + index) -- the device's finish record,
    or the host loop's in the same form -- of a call that kept n_gen steps."""
    rec = torch.as_tensor(record).to(torch.int64).cpu()
    kept = torch.where(rec[:, 0] >= 0, rec[:, 0] + 1, torch.full_like(rec[:, 0], n_gen)).clamp(max=n_gen)
    names = {REASON_NONE: "length", REASON_EOS: "eos", REASON_STOP: "stop"}
    reason = [names[int(c) >> 8] if int(f) >= 0 else "length" for f, c in rec.tolist()]
    index = [int(c) & 255 if int(f) >= 0 else -1 for f, c in rec.tolist()]
    return Finish(kept, reason, index)


# ------------------------------------------------------------------------------------------------- speculative greedy decoding
MAX_SPEC_TOKENS, MAX_SPEC_NGRAM, MAX_SPEC_ROWS = 7, 16, 16


class EngineOnlySpeculation(NotImplementedError, ValueError):
    """Speculation asked of an LM object without the HIP engine for something only the engine's launches do (sampled rows, stop
    sequences): not implemented for that LM, and a value the call cannot take -- callers that catch either class see it."""


class Speculation(NamedTuple):
    """What speculation did for every row of a generate() call (``return_speculation=True``): CPU int64 [B] each."""
    steps: torch.Tensor         # model calls in which the row was open, the prefill included
    drafted: torch.Tensor       # draft tokens fed
    accepted: torch.Tensor      # draft tokens the model agreed with


def prompt_lookup(ids, num_tokens: int, max_ngram: int, eos_ids=(), vocab: int = None) -> List[int]:
    """The draft of prompt-lookup decoding, the rule of transformers' ``PromptLookupCandidateGenerator.get_candidates``
    (``prompt_lookup_num_tokens`` / ``max_matching_ngram_size``): for n from min(max_ngram, len - 1) down to 1, the first window
    from the left that equals the last n tokens of ``ids`` and has a non-empty continuation inside ``ids`` decides: its
    continuation, at most ``num_tokens`` long, cut in front of the first eos id (``vocab``: or id outside [0, vocab)), is the
    draft -- possibly empty, no further window is tried then.  No window: no draft."""
    ids = [int(t) for t in (ids.tolist() if hasattr(ids, "tolist") else ids)]
    L, eos = len(ids), {int(e) for e in eos_ids}
    for n in range(min(int(max_ngram), L - 1), 0, -1):
        tail = ids[L - n:]
        for i in range(L - n):                      # i + n < L: the continuation is not empty
            if ids[i:i + n] == tail:
                draft = []
                for t in ids[i + n:min(i + n + int(num_tokens), L)]:
                    if t in eos or (vocab is not None and not 0 <= t < vocab):
                        break
                    draft.append(t)
                return draft
    return []


def speculate_update(ids, n_draft, token, history, count, finish, pos, stats, lookup, lookup_len, state, *, num_tokens: int,
                     max_ngram: int, eos_ids, limit: int, arm: bool = False, vocab: int = None, stop_seqs=()):
    """The bookkeeping of a speculative step, host statement (the device kernel is csrc/sampling.hip, spec_finish_kernel), IN
    PLACE on CPU tensors.  The step fed ``ids`` (B, T) int64 -- ids[b, 0] the row's last emitted token, ids[b, 1:1 + n_draft[b]]
    its drafts -- and ``token`` (B * T,) int64 holds the argmax of every fed row (``arm``: (B,), the prefill's selected tokens;
    nothing was fed, ``n_draft`` counts as 0 and ``pos`` stays).  Per row b with finish[b, 0] < 0:
      accept  a = the leading j in [1, n_draft[b]] with ids[b, j] == token[b * T + j - 1]; token[b * T + 0 .. a] are emitted, cut
              behind the first of ``eos_ids`` among them (finish[b] = (count, STOP_EOS | i)) and at min(limit, history columns) -
              count[b] (finish[b] = (count, STOP_LEN)).  ``stop_seqs``: stop_update's rule token by token -- emitted token j is
              recorded, tested against the eos ids first, then history[b, :count[b] + j + 1] against every sequence (one longer
              than that cannot match; the lowest matching index i wins: STOP_SEQ | i); the finishing token is kept, emission is
              cut behind it.  A draft that completes a sequence is accepted like any other: drafts are cut in front of eos ids only;
      record  the m emitted tokens go to history[b, count[b]:], count[b] += m, pos[b] += m, stats[b] += (1, n_draft, a);
      draft   a row still open: ids[b, 0] = its last emitted token, ids[b, 1:] = prompt_lookup(lookup[b, :lookup_len[b]] ++
              history[b, :count[b]], num_tokens, max_ngram, eos_ids), n_draft[b] their number, unused entries repeat ids[b, 0].
    A finished row (now or earlier) is frozen: n_draft[b] = 0, ids[b] = eos_ids[0], nothing else of it moves.  state[1] latches
    state[0] when no row is open; state[0] += 1.  Degenerate values: n_draft counts as clamped into [0, T - 1] (0 when arming),
    lookup_len into [0, lookup columns]; a row whose count lies outside [0, history columns] is skipped whole."""
    from .ops import STOP_EOS, STOP_LEN, STOP_SEQ
    B, T = ids.shape
    cols, lcols, ts = history.shape[1], lookup.shape[1], 1 if arm else T
    eos_ids = [int(e) for e in eos_ids]
    stop_seqs = [[int(t) for t in q] for q in stop_seqs]
    any_open = False
    for b in range(B):
        c = int(count[b])
        if int(finish[b, 0]) >= 0:
            n_draft[b], ids[b] = 0, eos_ids[0]
            continue
        if not 0 <= c <= cols:
            continue
        nd = max(0, min(int(n_draft[b]), min(T, ts) - 1))
        tk = [int(t) for t in token[b * ts:b * ts + nd + 1]]
        a = 0
        while a < nd and int(ids[b, a + 1]) == tk[a]:
            a += 1
        lim, m, code = min(int(limit), cols), 0, 0
        for j in range(a + 1):
            if c + j >= lim or code:
                break
            history[b, c + j], m = tk[j], j + 1
            if tk[j] in eos_ids:
                code = STOP_EOS | eos_ids.index(tk[j])
                continue
            n = c + j + 1
            for i, q in enumerate(stop_seqs):
                if 1 <= len(q) <= n and [int(t) for t in history[b, n - len(q):n]] == q:
                    code = STOP_SEQ | i
                    break
        if not code and c + m >= lim:
            code = STOP_LEN
        count[b] = c + m
        if pos is not None and not arm:
            pos[b] += m
        stats[b, 0] += 1
        stats[b, 1] += nd
        stats[b, 2] += a
        if code:
            finish[b, 0], finish[b, 1], n_draft[b], ids[b] = c + m, code, 0, eos_ids[0]
            continue
        any_open = True
        llen = max(0, min(int(lookup_len[b]), lcols))
        draft = prompt_lookup(lookup[b, :llen].tolist() + history[b, :c + m].tolist(), min(num_tokens, T - 1), max_ngram, eos_ids,
                              vocab)
        last = int(history[b, c + m - 1])
        ids[b] = last
        ids[b, 1:1 + len(draft)] = torch.tensor(draft, dtype=ids.dtype)
        n_draft[b] = len(draft)
    if not any_open and int(state[1]) < 0:
        state[1] = int(state[0])
    state[0] += 1


def crop_past(past, length: int):
    """A KV cache cut back to its first ``length`` positions (the rejected drafts of a speculative step leave it): transformers
    Cache objects (crop), or nested lists / tuples of (batch, heads, positions, dim) tensors."""
    if hasattr(past, "crop"):
        past.crop(length)
        return past
    if isinstance(past, (list, tuple)):
        return type(past)(crop_past(p, length) for p in past)
    if torch.is_tensor(past):
        return past[..., :length, :]
    raise TypeError(f"cannot crop a cache of type {type(past).__name__} for speculative decoding")


def check_speculation_args(prompt_lookup_num_tokens=0, max_matching_ngram_size=2, lookup_ids=None, return_speculation=False,
                           batch: int = None, vocab: int = None, encode: Callable = None):
    """ValueError for speculation arguments generate() does not take (NotImplementedError: more than 16 rows per step).  Returns
    None when the call does not speculate
    (``prompt_lookup_num_tokens`` = 0), else dict(T = drafts + 1 rows per sequence, max_ngram, lookup = None or ``batch`` lists of
    token ids).  ``prompt_lookup_num_tokens`` in [0, 7], ``max_matching_ngram_size`` in [1, 16]; ``lookup_ids``: one list of ids,
    tensor or string (``encode`` turns it into ids) per row, every id in [0, vocab); B * T may not exceed 16."""
    k, n = prompt_lookup_num_tokens, max_matching_ngram_size
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= MAX_SPEC_TOKENS:
        raise ValueError(f"prompt_lookup_num_tokens must be an integer in [0, {MAX_SPEC_TOKENS}] (0: off), got {k!r}")
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_SPEC_NGRAM:
        raise ValueError(f"max_matching_ngram_size must be an integer in [1, {MAX_SPEC_NGRAM}], got {n!r}")
    if k == 0:
        if lookup_ids is not None or return_speculation:
            raise ValueError("lookup_ids / return_speculation belong to speculative decoding: set prompt_lookup_num_tokens >= 1")
        return None
    if batch is not None and batch * (k + 1) > MAX_SPEC_ROWS:
        raise NotImplementedError(f"a speculative step runs B * (prompt_lookup_num_tokens + 1) rows and takes at most {MAX_SPEC_ROWS}: "
                         f"got {batch} * {k + 1} = {batch * (k + 1)}")
    rows = None
    if lookup_ids is not None:
        if isinstance(lookup_ids, str) or not isinstance(lookup_ids, (list, tuple)):
            raise ValueError("lookup_ids must be a list with one entry (token ids or a string) per row")
        if batch is not None and len(lookup_ids) != batch:
            raise ValueError(f"lookup_ids has {len(lookup_ids)} entries, the batch {batch} rows")
        rows = []
        for r, q in enumerate(lookup_ids):
            if isinstance(q, str):
                if encode is None:
                    raise ValueError(f"lookup_ids[{r}] is text and this model has no tokenizer to encode it")
                q = encode(q)
            if torch.is_tensor(q):
                q = q.flatten().tolist()
            if not isinstance(q, (list, tuple)):
                raise ValueError(f"lookup_ids[{r}] must be a list of token ids, a tensor or a string, got {q!r}")
            for t in q:
                if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
                    raise ValueError(f"lookup_ids[{r}] must hold token ids in [0, {'V' if vocab is None else vocab}), got {t!r}")
            rows.append([int(t) for t in q])
    return dict(T=k + 1, max_ngram=n, lookup=rows)


MAX_TOP_LOGPROBS = 20


class TokenLogprobs(NamedTuple):
    """Per-token log-probabilities of a generate() call (``return_logprobs=True``) or of Magma.score(): CPU tensors over the n
    generated (scored) columns.  Positions at or past ``count[b]`` hold 0.0 / -1 / -inf."""
    tokens: torch.Tensor        # int64 [B, n]
    logprobs: torch.Tensor      # fp32 [B, n]: log p(tokens[b, i]) under the raw model distribution of that step
    top_ids: torch.Tensor       # int64 [B, n, k]: the k most probable tokens of the step (raw logit descending, lower id first)
    top_logprobs: torch.Tensor  # fp32 [B, n, k]
    count: torch.Tensor         # int64 [B]: the positions of the row that count


def check_logprob_args(return_logprobs=False, top_logprobs=0, vocab: int = None):
    """ValueError for log-probability arguments generate() / score() do not take.  Returns None (off: nothing is launched or
    allocated) or n_top, the number of alternatives per token (0: the token's own log-probability only)."""
    k = top_logprobs
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= MAX_TOP_LOGPROBS:
        raise ValueError(f"top_logprobs must be an integer in [0, {MAX_TOP_LOGPROBS}], got {k!r}")
    if vocab is not None and k > vocab:
        raise ValueError(f"top_logprobs = {k} exceeds the vocabulary (V = {vocab})")
    if not isinstance(return_logprobs, bool):
        raise ValueError(f"return_logprobs must be True or False, got {return_logprobs!r}")
    return k if (return_logprobs or k > 0) else None


def token_logprobs(logits, tokens, n_top: int = 0):
    """Token log-probabilities, host statement (the device kernel is csrc/sampling.hip, token_logprobs_kernel) in float64:
    ``logits`` (R, V), ``tokens`` (R,) -> (log_softmax(logits)[r, tokens[r]] (R,) -- -inf for a token outside [0, V) --,
    top ids (R, n_top) int64 -- a STABLE descending sort of the logits: raw logit descending, lower id first --, their
    log-probabilities (R, n_top)), both values float64."""
    x = torch.as_tensor(logits).detach().cpu().to(torch.float64)
    t = torch.as_tensor(tokens).detach().cpu().to(torch.int64).view(-1)
    R, V = x.shape
    if not 0 <= int(n_top) <= min(MAX_TOP_LOGPROBS, V):
        raise ValueError(f"n_top must lie in [0, min({MAX_TOP_LOGPROBS}, V = {V})], got {n_top!r}")
    ls = F.log_softmax(x, dim=-1)
    ok = (t >= 0) & (t < V)
    lp = torch.where(ok, ls.gather(1, t.clamp(0, V - 1)[:, None])[:, 0], torch.full((R,), float("-inf"), dtype=torch.float64))
    ids = torch.sort(x, dim=-1, descending=True, stable=True)[1][:, : int(n_top)]
    return lp, ids, ls.gather(1, ids)


def mask_logprobs(tokens, lp, top_ids, top_lp, count) -> TokenLogprobs:
    """The result type from per-step values: positions at or past count[b] become 0.0 / -1 / -inf."""
    count = torch.as_tensor(count).to(torch.int64).cpu().view(-1)
    lp, top_ids, top_lp = lp.cpu().float().clone(), top_ids.cpu().to(torch.int64).clone(), top_lp.cpu().float().clone()
    gone = torch.arange(lp.shape[1])[None, :] >= count[:, None]
    lp[gone] = 0.0
    top_ids[gone] = -1
    top_lp[gone] = float("-inf")
    return TokenLogprobs(tokens.cpu().to(torch.int64).clone(), lp, top_ids, top_lp, count)


MAX_BEAMS = 16


def check_group_args(num_beams: int, num_beam_groups=1, diversity_penalty=0.0, vocab: int = None):
    """ValueError for group arguments diverse beam search does not take (num_beams already checked); returns
    (num_beam_groups, diversity_penalty as a float)."""
    G = num_beam_groups
    if isinstance(G, bool) or not isinstance(G, int) or G < 1:
        raise ValueError(f"num_beam_groups must be an integer >= 1, got {G!r}")
    if num_beams % G:
        raise ValueError(f"num_beam_groups must divide num_beams = {num_beams}, got {G}")
    lam = diversity_penalty
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(lam) or lam < 0:
        raise ValueError(f"diversity_penalty must be a finite number >= 0, got {lam!r}")
    if G == 1 and lam != 0:
        raise ValueError(f"diversity_penalty = {lam} needs num_beam_groups > 1: one group is never penalised")
    if vocab is not None and G > 1 and vocab < num_beams + num_beams // G:
        raise ValueError(f"num_beams = {num_beams} in {G} groups needs a vocabulary of at least {num_beams + num_beams // G} "
                         f"tokens, got {vocab}")
    return G, float(lam)


def check_beam_args(num_beams: int, num_return_sequences: int, early_stopping, num_beam_groups=1, diversity_penalty=0.0,
                    vocab: int = None):
    """ValueError for arguments beam search does not take; returns early_stopping normalised to True / False / "never"."""
    if not isinstance(num_beams, int) or num_beams < 1:
        raise ValueError(f"num_beams must be an integer >= 1, got {num_beams!r}")
    if num_beams > MAX_BEAMS:
        raise ValueError(f"num_beams must be at most {MAX_BEAMS}, got {num_beams}")
    if not isinstance(num_return_sequences, int) or num_return_sequences < 1 or num_return_sequences > num_beams:
        raise ValueError(f"num_return_sequences must lie in [1, num_beams = {num_beams}], got {num_return_sequences!r}")
    check_group_args(num_beams, num_beam_groups, diversity_penalty, vocab)
    if isinstance(early_stopping, str):
        if early_stopping != "never":
            raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        return early_stopping
    if early_stopping not in (True, False):
        raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
    return bool(early_stopping)


def reorder_past(past, rows: torch.Tensor):
    """A KV cache whose batch rows are rearranged by ``rows`` (row b <- old row rows[b]): transformers Cache objects
    (reorder_cache), or nested lists / tuples of (batch, ...) tensors."""
    if hasattr(past, "reorder_cache"):
        past.reorder_cache(rows)
        return past
    if isinstance(past, (list, tuple)):
        return type(past)(reorder_past(p, rows) for p in past)
    if torch.is_tensor(past):
        return past.index_select(0, rows.to(past.device))
    raise TypeError(f"cannot reorder a cache of type {type(past).__name__} for beam search")


class _BeamState:
    """The state of P (pseudo-)samples of k beams each in beam_search's rule: running scores (starting at [0, -1e9, ...]), the
    running and the finished token rows, the k finished slots and the early-stop latch."""

    def __init__(self, P: int, k: int, max_steps: int, eos_token: int):
        self.run = torch.zeros(P, k)
        self.run[:, 1:] = -1e9
        self.fin_score = torch.full((P, k), -1e9)
        self.fin_flag = torch.zeros(P, k, dtype=torch.bool)
        self.fin_len = torch.zeros(P, k, dtype=torch.int64)
        self.seq = torch.full((P, k, max_steps), eos_token, dtype=torch.int64)
        self.fin_seq = self.seq.clone()
        self.unsat = torch.ones(P, 1, dtype=torch.bool)


def _beam_rule(st: _BeamState, flat, t: int, V: int, max_steps: int, eos_token: int, length_penalty: float, early_stopping,
               record: list = None, extra: Callable = None, ties_by_index: bool = False):
    """One step of beam search's rule over ``st``'s P (pseudo-)samples of k beams, from their candidate scores ``flat``
    (P, k*V) fp32: the per-step arithmetic beam_search and group_beam_search share.  Advances ``st`` in place and returns
    (parent (P, k) -- the beam, within its sample, that each new running beam continues --, hits (P, 2k) -- which of the top
    candidates met a stopping criterion).  ``extra(top_s, beam, tok, nxt)``: further entries of the step's ``record`` dict.
    ``ties_by_index``: running beams of equal score are taken in candidate order, as the device takes them -- at the last step
    every candidate finishes and all of them round to -1e9, so the "running" beams are then the k best candidates.  Nothing
    reads them in beam search; in diverse beam search the later groups' penalty does."""
    P, k = st.run.shape
    K2 = 2 * k
    top_mask = torch.arange(K2) < k
    top_s, top_i = torch.topk(flat, K2)
    beam, tok = top_i // V, top_i % V
    cand_seq = torch.take_along_dim(st.seq, beam[:, :, None], dim=1)
    cand_seq[:, :, t] = tok
    hits = (tok == eos_token) | (t + 1 >= max_steps)
    # running beams: the best k that did not finish
    mod = top_s + hits.to(torch.float32) * -1.0e9
    nxt = torch.sort(mod, dim=1, descending=True, stable=True)[1][:, :k] if ties_by_index else torch.topk(mod, k)[1]
    st.seq = torch.take_along_dim(cand_seq, nxt[:, :, None], dim=1)
    st.run = torch.take_along_dim(mod, nxt, dim=1)
    parent = torch.take_along_dim(beam, nxt, dim=1)
    # finished slots
    just = hits & top_mask[None, :]
    v = top_s / ((t + 1) ** length_penalty)
    v += (torch.all(st.fin_flag, dim=-1, keepdim=True) & (early_stopping is True)).to(torch.float32) * -1.0e9
    v += (~st.unsat).to(torch.float32) * -1.0e9
    v += (~just) * -1.0e9
    m_score = torch.cat((st.fin_score, v), dim=1)
    pick = torch.topk(m_score, k)[1]
    st.fin_seq = torch.take_along_dim(torch.cat((st.fin_seq, cand_seq), dim=1), pick[:, :, None], dim=1)
    st.fin_score = torch.take_along_dim(m_score, pick, dim=1)
    st.fin_flag = torch.take_along_dim(torch.cat((st.fin_flag, just), dim=1), pick, dim=1)
    st.fin_len = torch.take_along_dim(torch.cat((st.fin_len, torch.full((P, K2), t + 1)), dim=1), pick, dim=1)
    # early-stop heuristic (latched)
    hyp = max_steps if (early_stopping == "never" and length_penalty > 0.0) else t + 1
    best = st.run[:, :1] / (hyp ** length_penalty)
    worst = torch.where(st.fin_flag, torch.min(st.fin_score, dim=1, keepdim=True)[0], -1.0e9)
    if record is not None:
        record.append(dict(top=torch.topk(flat, min(K2 + 1, k * V)).values, merged=m_score, best=best.clone(),
                           worst=worst.clone(), unsat=st.unsat.clone(), finished=just.clone(),
                           eos_outside=(tok[:, k:] == eos_token).clone(), step=t,
                           **(extra(top_s, beam, tok, nxt) if extra is not None else {})))
    st.unsat = st.unsat & torch.any(best > worst, dim=-1, keepdim=True)
    return parent, hits


@torch.no_grad()
def beam_search(step: Callable, batch_size: int, num_beams: int, max_steps: int, eos_token: int, length_penalty: float = 1.0,
                early_stopping=False, num_return_sequences: int = 1, record: list = None, processors: dict = None):
    """Beam search, the rule of transformers' vectorised ``GenerationMixin._beam_search`` called with do_sample=False, one eos
    id and the prompt passed as embeddings (prompt length 0: lengths count generated tokens only), in the same fp32 torch
    arithmetic.  This is the host statement the device kernels (csrc/sampling.hip, beam_*) are tested against.

    ``step(parents, tokens)`` returns the fp32 logits (B*k, V) of the running rows (sample-major, k = num_beams): first
    ``step(None, None)`` (the prompts, each repeated k times), then ``parents`` (B*k,) int64 -- the row each new row
    continues, its cache must be reordered so -- and ``tokens`` (B*k,), the last token of each row.

    Per step and sample: the top 2k of the k*V candidates running_score[beam] + log_softmax(logits[beam]) (running scores
    start at [0, -1e9, ...]: the first step expands beam 0 only); a candidate among the first k that ends in eos (or reaches
    max_steps) finishes with score sum_logprobs / gen_len ** length_penalty and merges into the k finished slots; the best k
    that do not end in eos run on.  early_stopping True: a sample stops taking hypotheses once its k slots are full; False:
    once the best running beam, scored at the current length, cannot beat the worst finished one; "never": the same at
    max_steps when length_penalty > 0.

    Returns (sequences (B*n_ret, n) int64, eos-padded, n = the longest returned hypothesis; scores (B*n_ret,) fp32;
    lengths (B*n_ret,) int64), the best n_ret = num_return_sequences hypotheses per sample in score order.

    ``record`` (a list): one dict per step is appended with the values every decision of that step compared -- the top 2k + 1
    candidate scores per sample, the merged finished-slot scores, the early-stop comparison and whether a candidate finished
    or hit eos outside the first k -- for beam_margin() and for tests that must show which rules a run exercised.

    ``processors`` (check_processor_args' dict, or None): the logits processors, applied as transformers' _beam_search applies
    them -- to log_softmax(logits) of every row, with the row's tokens so far, before the running score is added and without
    renormalising."""
    early_stopping = check_beam_args(num_beams, num_return_sequences, early_stopping)
    B, k = batch_size, num_beams
    st = _BeamState(B, k, max_steps, eos_token)
    logits = step(None, None)
    for t in range(max_steps):
        V = logits.shape[-1]
        lp = F.log_softmax(logits.float().cpu(), dim=-1)
        if processors:
            lp = process_logits(lp, st.seq.reshape(B * k, max_steps), t, eos_token=eos_token, **processors)
        lp = lp.view(B, k, V) + st.run[:, :, None]
        parent, hits = _beam_rule(st, lp.reshape(B, k * V), t, V, max_steps, eos_token, length_penalty, early_stopping, record)
        # the stop rule of the whole batch
        go_on = (bool(torch.any(st.unsat)) and not (bool(torch.all(st.fin_flag)) and early_stopping is True)
                 and not bool(torch.all(hits)))
        if not go_on:
            break
        rows = (parent + torch.arange(B)[:, None] * k).reshape(-1)
        logits = step(rows, st.seq[:, :, t].reshape(-1))
    n_ret = num_return_sequences
    lens = st.fin_len[:, :n_ret].reshape(-1)
    n = int(lens.max())
    return st.fin_seq[:, :n_ret, :n].reshape(B * n_ret, n), st.fin_score[:, :n_ret].reshape(-1).clone(), lens


@torch.no_grad()
def group_beam_search(step: Callable, batch_size: int, num_beams: int, num_beam_groups: int, diversity_penalty: float,
                      max_steps: int, eos_token: int, length_penalty: float = 1.0, early_stopping=False,
                      num_return_sequences: int = 1, record: list = None, processors: dict = None):
    """Diverse beam search (Vijayakumar et al., "Diverse Beam Search", 2018), stated from the paper in beam_search's fp32
    torch arithmetic (``_beam_rule``): the host statement mg_beam_finish_groups is tested against (DESIGN.md "Diverse beam
    search").  k = num_beams beams in G = num_beam_groups groups of k' = k / G; the rows ``step`` sees are sample-major, then
    group-major: row b*k + g*k' + q.

    A group is a pseudo-sample: group (b, g) runs beam_search's rule with k' beams over its own rows -- its own running scores
    (starting at [0, -1e9, ...]), its own k' finished slots, its own early-stop latch, its own top 2k' candidates.  The call
    stops by beam_search's rule over the B*G groups; a group whose latch has dropped keeps running beams, as samples do.

    Within a step the groups of a sample are handled in the order g = 0 .. G-1, and group g's candidate scores are
    (run + logp) - lambda * n_t in fp32: run + logp is beam_search's candidate, lambda * n_t one rounded product, the
    subtraction one rounded subtraction.  n_t counts the running beams of groups 0 .. g-1 of the same sample whose token
    selected AT THIS STEP is t (whether or not their latch has dropped); group 0 is never penalised; -inf stays -inf.  At the
    last step, where every candidate finishes and the running scores all round to -1e9, a group's "running" beams are its k'
    best candidates (ties are taken in candidate order), so the tokens its hypotheses end in are penalised like any other.
    ``processors`` run first, on log_softmax, as in beam_search; the diversity term comes after them, on the candidate score.

    Returns beam_search's triple; the n_ret = num_return_sequences (in [1, k]) hypotheses of a sample are taken round-robin
    over the groups by rank within each group -- g0's best, g1's best, ..., g(G-1)'s best, g0's second, ... -- each with its own
    score: n_ret = G is one hypothesis per group, n_ret = 1 is group 0's best (plain beam search with k' beams).

    ``record``: one dict per step AND group is appended (group-minor), holding what beam_search records per sample -- taken on
    the penalised scores, so beam_margin reads it as it is -- and ``group``; ``counts`` (B, V), n_t as the group saw it;
    ``top_beam`` / ``top_tok`` / ``top_n`` (B, 2k'), the group's top candidates and their n_t; ``running`` (B, k'), which of
    them became its running beams; ``row_rank`` (B, 2k'), the position of each top candidate in its own row's UNPENALISED order
    (score descending, lower token first): a value >= 2k' is a candidate that lists of 2k' per row would have missed, and
    k + k' - 1 -- the last entry of the device's lists -- is the largest there can be."""
    early_stopping = check_beam_args(num_beams, num_return_sequences, early_stopping, num_beam_groups, diversity_penalty)
    B, k, G = batch_size, num_beams, num_beam_groups
    kq = k // G
    lam = torch.tensor(float(diversity_penalty), dtype=torch.float32)
    groups = [_BeamState(B, kq, max_steps, eos_token) for _ in range(G)]
    logits = step(None, None)
    for t in range(max_steps):
        V = logits.shape[-1]
        if V < k + kq:
            raise ValueError(f"num_beams = {k} in {G} groups needs a vocabulary of at least {k + kq} tokens, got {V}")
        lp = F.log_softmax(logits.float().cpu(), dim=-1)
        if processors:
            seq = torch.stack([st.seq for st in groups], dim=1)                      # (B, G, k', max_steps)
            lp = process_logits(lp, seq.reshape(B * k, max_steps), t, eos_token=eos_token, **processors)
        lp = lp.view(B, G, kq, V)
        counts = torch.zeros(B, V, dtype=torch.float32)
        parents, all_hits = [], []
        for g, st in enumerate(groups):
            plain = lp[:, g] + st.run[:, :, None]                                    # beam_search's candidates (B, k', V)
            cand = plain - (lam * counts)[:, None, :]
            seen = counts.clone()

            def extra(top_s, beam, tok, nxt, g=g, plain=plain, seen=seen):
                row = torch.take_along_dim(plain, beam[:, :, None], dim=1)           # (B, 2k', V): the row each one came from
                mine = torch.take_along_dim(row, tok[:, :, None], dim=2)
                before = (row > mine) | ((row == mine) & (torch.arange(V)[None, None, :] < tok[:, :, None]))
                return dict(group=g, counts=seen, top_n=torch.take_along_dim(seen, tok, dim=1), top_beam=beam.clone(),
                            top_tok=tok.clone(), running=nxt.clone(), row_rank=before.sum(-1))

            parent, hits = _beam_rule(st, cand.reshape(B, kq * V), t, V, max_steps, eos_token, length_penalty, early_stopping,
                                      record, extra if record is not None else None, ties_by_index=True)
            counts.scatter_add_(1, st.seq[:, :, t], torch.ones(B, kq))
            parents.append(parent + g * kq)
            all_hits.append(hits)
        # the stop rule of the whole call, over the B*G groups
        go_on = (any(bool(torch.any(st.unsat)) for st in groups)
                 and not (all(bool(torch.all(st.fin_flag)) for st in groups) and early_stopping is True)
                 and not all(bool(torch.all(h)) for h in all_hits))
        if not go_on:
            break
        rows = (torch.cat(parents, dim=1) + torch.arange(B)[:, None] * k).reshape(-1)
        logits = step(rows, torch.cat([st.seq[:, :, t] for st in groups], dim=1).reshape(-1))
    n_ret = num_return_sequences
    # round-robin over the groups by rank within the group: (B, G, k') -> (B, k', G) -> the first n_ret
    pool = lambda name: torch.stack([getattr(st, name) for st in groups], dim=1).transpose(1, 2)  # noqa: E731
    lens = pool("fin_len").reshape(B, k)[:, :n_ret].reshape(-1)
    n = int(lens.max())
    seqs = pool("fin_seq").reshape(B, k, max_steps)[:, :n_ret, :n].reshape(B * n_ret, n)
    return seqs, pool("fin_score").reshape(B, k)[:, :n_ret].reshape(-1).clone(), lens


def beam_margin(record: list) -> float:
    """Smallest gap between two values that a decision of a recorded beam_search run compared: consecutive top-2k+1 candidate
    scores of a sample, consecutive real finished-slot scores, and the early-stop comparison (values at -1e9 are placeholders
    and are left out).  A run on other arithmetic (bf16 logits) makes the same decisions while its scores stay within half of
    this of the recorded ones."""
    gaps = [float("inf")]
    for r in record:
        for row in r["top"]:
            v = row[row > -1e8]
            if v.numel() > 1:
                gaps.append(float((v[:-1] - v[1:]).min()))
        for row in r["merged"]:
            v = torch.sort(row[row > -1e8], descending=True).values
            if v.numel() > 1:
                gaps.append(float((v[:-1] - v[1:]).min()))
        live = r["unsat"][:, 0] & (r["worst"] > -1e8).all(-1)
        if bool(live.any()):
            gaps.append(float((r["best"][live] - r["worst"][live].min(-1, keepdim=True).values).abs().min()))
    return min(gaps)


def check_contrastive_args(penalty_alpha=0.0, top_k=0, vocab: int = None):
    """ValueError for arguments contrastive search does not take; returns None when it is off (``penalty_alpha`` == 0: ``top_k``
    is then the sampler's keyword and is not looked at), else (top_k, penalty_alpha as a float)."""
    a = penalty_alpha
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or not 0.0 <= a <= 1.0:
        raise ValueError(f"penalty_alpha must be a finite number in [0, 1] (0 = contrastive search off), got {a!r}")
    if a == 0:
        return None
    k = top_k
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"top_k must be an integer in [1, {MAX_BEAMS}] with penalty_alpha > 0, got {k!r}")
    if k == 0:
        raise ValueError(f"penalty_alpha = {a} needs top_k candidates: pass top_k in [1, {MAX_BEAMS}] (transformers' examples use 4)")
    if not 1 <= k <= MAX_BEAMS:
        raise ValueError(f"top_k must be an integer in [1, {MAX_BEAMS}] with penalty_alpha > 0, got {k!r}")
    if vocab is not None and k > vocab:
        raise ValueError(f"top_k = {k} exceeds the vocabulary of {vocab} tokens")
    return k, float(a)


def contrastive_rank(context, ctx_len, cand_hidden, cand_p, penalty_alpha: float):
    """Steps 3-4 of contrastive search's rule for B samples, in fp64: ``context`` (B, T, d) the context hidden states, of which
    the first ``ctx_len[b]`` count; ``cand_hidden`` (B, k, d) and ``cand_p`` (B, k) the candidates' hidden states and
    probabilities.  penalty_j = max over the valid c of cos(h_j, c) (a zero vector gives cosine 0; no valid position gives 0),
    score_j = (1 - penalty_alpha) * p_j - penalty_alpha * penalty_j.  Returns (selected (B,) int64: the first j with the largest
    score, score (B, k) fp64, penalty (B, k) fp64).  The host statement mg_contrastive_sim_bf16 / mg_contrastive_finish are
    tested against."""
    c, h = context.detach().cpu().double(), cand_hidden.detach().cpu().double()
    ctx_len = torch.as_tensor(ctx_len).cpu().to(torch.int64)
    den = h.norm(dim=-1)[:, :, None] * c.norm(dim=-1)[:, None, :]
    cos = torch.einsum("bkd,btd->bkt", h, c)
    cos = torch.where(den > 0, cos / den.clamp_min(1e-300), torch.zeros_like(cos))
    valid = torch.arange(c.shape[1])[None, :] < ctx_len[:, None]
    cos = cos.masked_fill(~valid[:, None, :], -math.inf)
    pen = cos.max(dim=-1).values if c.shape[1] else torch.full(h.shape[:2], -math.inf, dtype=torch.float64)
    pen = torch.where(torch.isinf(pen), torch.zeros_like(pen), pen)
    score = (1.0 - penalty_alpha) * cand_p.detach().cpu().double() - penalty_alpha * pen
    return torch.argmax(score, dim=-1), score, pen


@torch.no_grad()
def contrastive_search(step: Callable, prompt_hidden, first_logits, lengths, top_k: int, penalty_alpha: float, max_steps: int,
                       eos_token: int, stop_on_eos: bool = True):
    """Contrastive search (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; ``penalty_alpha`` / ``top_k`` of
    transformers 4.x's ``generate``), stated from the paper: the host statement the device kernels (csrc/sampling.hip,
    contrastive_*) are tested against.

    Per sample a list C of context hidden states -- ``prompt_hidden`` (B, S, d), of which the first ``lengths[b]`` count (None: all
    S), then one per generated token.  Per step: p = softmax(logits) in fp32 of the last context position (``first_logits``
    (B, V), then the selected candidate's); the candidates are the ``top_k`` most probable tokens, ordered by descending
    probability, ties by smaller id (taken on the logits, which p is monotone in); ``step`` forwards them; the candidate with the
    first largest (1 - alpha) * p_j - alpha * max_{c in C} cos(h_j, c) (``contrastive_rank``) is emitted, its hidden state joins C,
    its logits are the next step's.  Every generated token costs one ``step``, the first included.  With ``stop_on_eos`` the loop
    ends after the first step at which every sample emitted ``eos_token`` (greedy decoding's rule).

    ``step(tokens, parents)`` returns (fp32 logits (B*k, V), hidden states (B*k, d)) of the candidate ``tokens`` (B*k,) int64,
    sample-major, each forwarded against the cache as it stands.  ``parents`` is None on the first call and afterwards (B*k,)
    int64: the row of the PREVIOUS call whose K / V every row now continues (b*k + the selected j, k times per sample) -- the
    callback owns the cache, as in beam_search.

    Returns (tokens (B, n) int64, record): one dict per step with ``cand`` (B, k) ids, ``p``, ``penalty``, ``score`` (B, k),
    ``selected`` (B,) and ``gap`` (B,), the best score less the second best (inf at top_k = 1), for contrastive_margin()."""
    top_k, penalty_alpha = check_contrastive_args(penalty_alpha, top_k, first_logits.shape[-1])
    B, V = first_logits.shape
    k = top_k
    hid = prompt_hidden.detach().cpu()
    S, d = hid.shape[1], hid.shape[2]
    ctx = torch.zeros(B, S + max_steps, d, dtype=hid.dtype)
    ctx[:, :S] = hid
    ctx_len = torch.full((B,), S, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths).cpu().to(torch.int64).clone()
    logits = first_logits.detach().float().cpu()
    rows = torch.arange(B)
    tokens, record, parents = [], [], None
    for _ in range(max_steps):
        p = F.softmax(logits, dim=-1)
        cand = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]
        cand_p = torch.take_along_dim(p, cand, dim=1)
        lg, h = step(cand.reshape(-1), parents)
        lg, h = lg.detach().float().cpu().view(B, k, V), h.detach().cpu().view(B, k, d)
        sel, score, pen = contrastive_rank(ctx, ctx_len, h, cand_p, penalty_alpha)
        top2 = torch.topk(score, min(2, k), dim=-1).values
        gap = top2[:, 0] - top2[:, 1] if k > 1 else torch.full((B,), math.inf, dtype=torch.float64)
        record.append(dict(cand=cand, p=cand_p, penalty=pen, score=score, selected=sel, gap=gap))
        tok = cand[rows, sel]
        ctx[rows, ctx_len] = h[rows, sel].to(ctx.dtype)
        ctx_len += 1
        logits = lg[rows, sel]
        parents = (rows * k + sel).repeat_interleave(k)
        tokens.append(tok)
        if stop_on_eos and eos_token is not None and bool((tok == eos_token).all()):
            break
    return (torch.stack(tokens, 1) if tokens else torch.zeros(B, 0, dtype=torch.int64)), record


def contrastive_margin(record: list) -> float:
    """Smallest gap between the best and the second-best score of any sample at any step of a recorded contrastive_search run.  A
    run on other arithmetic makes the same selections while its scores stay within half of this of the recorded ones."""
    return min([float("inf")] + [float(r["gap"].min()) for r in record])


def _logit_count(model):
    """V, the number of logits of the model's LM (rows of lm_head), or None when the LM object does not say."""
    cfg = getattr(getattr(model, "lm", None), "config", None)
    v = getattr(cfg, "head_rows", None) or getattr(cfg, "vocab_size", None)
    return int(v) if isinstance(v, int) else None


@contextlib.contextmanager
def eval_mode(model):
    """The model in eval mode for the block; behind it -- after an exception too -- in the mode it was given in."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def poll_every(eos_check_every=None) -> int:
    """The steps between two host looks at the device's all-eos record: the argument, else MAGMA_EOS_CHECK_EVERY, else 8."""
    return eos_check_every or int(os.environ.get("MAGMA_EOS_CHECK_EVERY", "8"))


def sampling_mode(temperature, top_k, top_p, warp, seed):
    """(mode, seed): mode None (greedy), (temperature, top_k, top_p), or -- ``warp``: check_sampler_args' dict -- ("warp",
    temperature, top_k, top_p, min_p); a sampled call without a seed draws one from torch's CPU generator here."""
    if temperature == 0.0:
        return None, seed
    mode = (float(temperature), int(top_k), float(top_p))
    if warp is not None:
        mode = ("warp",) + mode + (warp["min_p"],)
    return mode, int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed


ROW_SAMPLER_ARGS = ("temperature", "top_k", "top_p", "min_p", "seed")


def per_row_given(**args) -> tuple:
    """The names among generate()'s ``temperature, top_k, top_p, min_p, seed`` that are given per row: a list, a tuple or a
    tensor / array of one dimension.  Empty: the call is the scalar one."""
    def is_seq(v):
        return isinstance(v, (list, tuple)) or (hasattr(v, "ndim") and hasattr(v, "tolist") and getattr(v, "ndim", 0) >= 1)
    return tuple(k for k in ROW_SAMPLER_ARGS if is_seq(args.get(k)))


def check_row_sampler_args(batch: int, sampler="reference", temperature=0.7, top_k=0, top_p=0.9, min_p=0.0, seed=None) -> list:
    """Per-row sampler settings (DESIGN.md "Per-request sampling"): each of the five may be a sequence or a one-dimensional tensor of
    ``batch`` values, a scalar stands for every row.  Returns one record (temperature, top_k, top_p, min_p, seed) per row, every
    row checked as the scalar call checks its arguments (check_sampler_args; min_p on a greedy row), with the bounds the flat
    kernels refuse; a sampled row without a seed draws one from torch's CPU generator, where the scalar call draws its own, and a
    greedy row's seed is 0 (it reads none).  A tensor's values are taken as they are: a float32 0.9 is not the double 0.9 the scalar
    call passes down, so pass float64 tensors (or lists) where a row must equal its scalar call."""
    cols = {}
    for name, v in zip(ROW_SAMPLER_ARGS, (temperature, top_k, top_p, min_p, seed)):
        if per_row_given(**{name: v}):
            v = v.tolist() if hasattr(v, "tolist") else list(v)
            if len(v) != batch:
                raise ValueError(f"{name} has {len(v)} entries, the batch {batch} rows: pass one value per row or a scalar")
        else:
            v = [v] * batch
        cols[name] = v
    rows = []
    for r in range(batch):
        t, k, p, m, sd = (cols[name][r] for name in ROW_SAMPLER_ARGS)
        where = f"row {r}: "
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0.0 <= t < float("inf"):
            raise ValueError(f"{where}temperature must be a finite number >= 0 (0: greedy), got {t!r}")
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < 2 ** 31:
            raise ValueError(f"{where}top_k must be an integer >= 0 (0: off), got {k!r}")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
            raise ValueError(f"{where}top_p must be a number in [0, 1], got {p!r}")
        try:
            check_sampler_args(sampler, m, p)
        except ValueError as e:
            raise ValueError(where + str(e)) from None
        if m > 0 and t == 0.0:
            raise ValueError(f"{where}min_p applies to sampled selection: greedy decoding (temperature=0) would drop it")
        if sd is not None and (isinstance(sd, bool) or not isinstance(sd, int)):
            raise ValueError(f"{where}seed must be an integer or None, got {sd!r}")
        if t == 0.0:
            sd = 0
        elif sd is None:
            sd = int(torch.randint(0, 2 ** 62, (1,)).item())
        rows.append((float(t), int(k), float(p), float(m), int(sd) & 0x7fffffffffffffff))
    return rows


def layout_ids(tokens, s: int, lengths, image_token: int, eos_token: int, repeat: int = 1):
    """The ids generate() returns, (rows, s + n) on the device of ``tokens`` (rows, n): per row the image token for the length of
    its prompt, its tokens, eos up to the width.  ``lengths``: None (every prompt is ``s`` long) or the samples' host int64
    lengths, each standing for ``repeat`` consecutive rows (the hypotheses beam search returns per sample)."""
    rows, n = tokens.shape
    dev = tokens.device
    out = torch.full((rows, s + n), eos_token, dtype=torch.long, device=dev)
    if lengths is not None:     # ragged: a row's tokens follow its own prompt, eos after them
        lens = lengths.to(dev, non_blocking=True)                   # (no host sync: the next call's launches queue behind this one)
        lens = (lens if repeat == 1 else lens.repeat_interleave(repeat))[:, None]
        out.masked_fill_(torch.arange(s + n, device=dev)[None, :] < lens, image_token)
        out.scatter_(1, lens + torch.arange(n, device=dev)[None, :], tokens)
    else:
        out[:, :s] = image_token
        out[:, s:] = tokens
    return out


def decode_ids(model, out, eos_token, s: int = 0, lengths=None, finish=None) -> List[str]:
    """``decode=True``: every row of ids as text -- by the reference's rule, cut at the first eos, image tokens dropped; with
    ``finish`` (a per-row call's Finish; ``s`` / ``lengths``: the prompts' width and lengths, as for layout_ids), the row's own
    kept tokens without the eos that finished it."""
    if finish is None:
        return [model.tokenizer.decode(remove_tokens_after_eos(row, eos_token, model.image_token)) for row in out]
    rows = []
    for r, at in enumerate(lengths.tolist() if lengths is not None else [s] * len(out)):
        ids = out[r, at: at + int(finish.kept[r])].tolist()
        rows.append(model.tokenizer.decode([t for t in (ids[:-1] if finish.reason[r] == "eos" else ids) if t != model.image_token]))
    return rows


@torch.no_grad()
def generate(model, embeddings, max_steps: int = 100, temperature: float = 0.7, top_k: int = 0,
             top_p: float = 0.9, eos_token: int = None, decode: bool = True,
             stop_on_eos: bool = True, seed: int = None, eos_check_every: int = None,
             lengths=None, num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False,
             num_return_sequences: int = 1, return_scores: bool = False, past_key_values=None,
             return_past_key_values: bool = False, *, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
             min_new_tokens: int = 0, suppress_tokens=None, stop_sequences=None, stop_per_row: bool = None,
             return_finish: bool = False, sampler: str = "reference", min_p: float = 0.0, return_logprobs: bool = False,
             top_logprobs: int = 0, constraint=None, guidance_scale: float = 1.0, negative_embeddings=None,
             negative_lengths=None, guidance_min_p: float = 0.0, num_beam_groups: int = 1,
             diversity_penalty: float = 0.0, penalty_alpha: float = 0.0, prompt_lookup_num_tokens: int = 0,
             max_matching_ngram_size: int = 2, lookup_ids=None,
             return_speculation: bool = False) -> Union[List[str], torch.Tensor]:
    """reference sampling.py:43-121.  Token selection (argmax, or top-k / the reference's top-p rule / softmax /
    multinomial) and the ``(next_token == eos).all()`` test run on the device inside the captured token step; the host
    reads the recorded "first all-eos step" every ``eos_check_every`` steps (default 8, MAGMA_EOS_CHECK_EVERY) instead of
    synchronising on every token, and cuts the output there -- same result as the reference's per-step break.
    ``seed`` fixes the sampling stream (default: drawn from torch's CPU generator, so torch.manual_seed reproduces a run).

    Ragged batches (prompts of different lengths): ``lengths`` (int [B]) gives the prompt length of every row of the
    right-padded ``embeddings`` (B, S_max, d); ``embeddings`` may also be a list of (1, s_i, d) / (s_i, d) tensors, padded
    here.  Row b of the output is then image_token x len_b, the generated tokens, eos up to the width S_max + n (n = steps
    run).  Needs the HIP engine (an LM object without device token selection raises).

    Beam search (``num_beams`` > 1, at most 16; DESIGN.md "Beam search"): the rule of transformers' ``_beam_search`` with
    do_sample=False (``beam_search`` above), ``length_penalty`` / ``early_stopping`` (True, False, "never") as there.
    temperature, top_k, top_p and seed do not apply.  Returns the best ``num_return_sequences`` hypotheses of every sample,
    sample-major: B * n_ret strings, or (B * n_ret, s + n) ids laid out as above (n = the longest returned hypothesis);
    ``return_scores=True`` returns (output, fp32 scores (B * n_ret,)) -- with num_beams=1 that runs the beam rule with one
    beam.  The HIP engine runs the whole beam step on the device; any other LM object runs the host statement.

    Diverse beam search (DESIGN.md "Diverse beam search"; Vijayakumar et al. 2018): ``num_beam_groups`` = G > 1 (a divisor of
    ``num_beams``) runs the beams in G groups of k' = num_beams / G, each by the beam rule with k' beams -- its own finished
    slots, its own early-stop latch --, and within a step group g scores a candidate token ``diversity_penalty`` (finite, >= 0,
    and 0 at G = 1; 0 at G > 1 gives G equal groups) lower for every beam of groups 0 .. g-1 of the same sample that selected
    that token at this step (``group_beam_search`` above), so the groups drift apart: several DIFFERENT captions of one image.
    The logits processors run first, on log_softmax; the diversity term comes after them, on the candidate score (transformers
    4.x put its Hamming processor in front of the repetition penalty).  The ``num_return_sequences`` hypotheses of a sample come
    back round-robin over the groups by rank within each group -- group 0's best, group 1's best, ..., then the second of
    each --, every one with its own score (transformers 4.x pooled them by score): n_ret = G is one caption per group, n_ret = 1
    is group 0's best, i.e. plain beam search with k' beams.  V must be at least num_beams + k'.  The HIP engine runs it in the
    same three launches per token as beam search (the candidate lists are num_beams + k' long, the bookkeeping launch walks the
    groups); any other LM object runs the host statement.  At ``num_beam_groups=1`` the call is bit for bit what it was.

    Multi-turn (DESIGN.md "Continuing from a cache"; HIP engine only, greedy or sampled): ``return_past_key_values=True`` returns
    (output, past).  ``past`` belongs to the caller (no later call reuses its buffers) and holds every row's conversation: its
    prompt and its generated tokens before its first eos.  ``generate(new, past_key_values=past)`` continues it with the new
    inputs -- a (B, T, d) tensor, a list of per-row tensors or embed_batch's (embeddings, lengths) -- and gives what a fresh call
    over [prompt_b ; kept tokens_b ; new_b] gives; only the new rows go through the blocks.  The output is laid out as for a call
    on the new inputs alone.  ``past`` is advanced in place; KVCache.expand(n) gives each row n copies (one cached prompt, n
    questions).  A continued call leaves ``past`` holding the whole conversation so far (the same state it returns with
    ``return_past_key_values=True``), so it can be continued again.

    Logits processors (DESIGN.md "Logits processors"; all three selection modes): ``repetition_penalty`` (> 0, 1.0 = off),
    ``no_repeat_ngram_size`` (0 = off, at most 16), ``min_new_tokens`` (eos is banned for that many steps) and
    ``suppress_tokens`` (at most 1024 ids that are never selected) are the rules of transformers' processors of those names
    (``process_logits`` above), applied in transformers' order to the raw logits before temperature / top-k / top-p, and in
    beam search to log_softmax(logits) before the running score is added.  The prompt is embeddings, so the rules see the
    tokens generated by THIS call only: a continued conversation (``past_key_values``) starts with an empty history again.
    The HIP engine applies them inside the captured token step (one small launch in front of the selection); at the
    defaults nothing is launched and the output is bit for bit what it was.

    Per-row stopping (DESIGN.md "Per-row stopping"; greedy and sampled): the rule of transformers' ``_sample`` (``stop_update``
    above) instead of the reference's -- a row that finished stays finished and is padded with ``eos_token[0]``, the call ends
    after the first step at which every row is finished, the output is s + that step + 1 wide.  ``eos_token`` may be a sequence
    of 1 to 8 ids (a row finishes on any of them; ``min_new_tokens`` bans every one).  ``stop_sequences``: at most 16 entries,
    each 1 to 16 token ids or a ``str`` that ``model.tokenizer.encode`` turns into ids; a row finishes when the tokens it
    generated IN THIS CALL end with one of them, and keeps them.  The match is over token ids: text that the model spells with
    other tokens is not found (unlike transformers' ``stop_strings``); ``min_new_tokens`` does not hold a stop sequence back.
    ``stop_per_row``: None = per-row exactly when ``eos_token`` is a sequence or ``stop_sequences`` is given; True with one eos
    id gives a plain batch the per-row rule (it ends when every row HAS emitted eos); False with either raises ValueError.
    ``stop_on_eos=False`` still runs all ``max_steps``: finished rows are padded, the output has a fixed width.
    ``return_finish=True`` returns (output, finish) -- (output, past, finish) with a cache --, ``finish`` a ``Finish``: ``kept``
    int64 [B] (the row's generated tokens that count, the finishing token included), ``reason`` ("eos" | "stop" | "length" per
    row) and ``index`` (which eos id / sequence).  ``decode=True`` then cuts every row at its own ``kept``.  The HIP engine runs
    the rule in the bookkeeping launch of the captured token step (no further launch, no host round trip); any other LM object
    runs the host statement.  Not combined with beam search (NotImplementedError).

    transformers' sampler (DESIGN.md "transformers' sampler"; sampled selection only): ``sampler="transformers"`` replaces the
    reference's filters -- whose top-p is not nucleus sampling and is usually a no-op (``top_p_filter``) -- by the rules of
    transformers' ``_sample`` with do_sample=True, applied after the logits processors in transformers' order: temperature,
    ``top_k`` (every tie at the k-th value stays; ``top_k_filter_ties``), nucleus ``top_p`` (the smallest set of most probable
    tokens whose mass reaches top_p at that temperature; 0 and 1 are off; ``nucleus_filter``) and ``min_p`` (tokens less
    probable than min_p times the most probable one go; 0 is off; ``min_p_filter``), then the same draw on the same stream.
    The HIP engine runs them in the selection launch of the captured token step (no further launch); any other LM object runs
    the host statements.  ``sampler="reference"`` (the default) is bit for bit what it was and takes no ``min_p``.  Greedy
    decoding and beam search ignore the sampler, and raise ValueError for ``min_p`` > 0.

    Constrained decoding (DESIGN.md "Constrained decoding"; greedy and sampled): ``constraint`` keeps every row's output inside
    a closed set of answers -- a ``TokenTrie``, a list of token-id sequences or strings (``model.tokenizer.encode`` turns a string
    into ids), or a list of B of either, one per row (multiple choice: other options for every question).  At every step a row may
    select only a token that continues one of its sequences, an eos id only where a sequence ends, and after that (or once it has
    left the trie) the eos ids alone: the rule of transformers' ``PrefixConstrainedLogitsProcessor`` over a trie
    (``constrain_logits`` above), applied with the logits processors -- after the repetition penalty, before temperature / top-k /
    top-p -- to the tokens generated by THIS call: a continued conversation starts at the root again.  The HIP engine applies it
    in the processor launch of the captured token step (with a constraint alone: one small launch more per token); any other LM
    object runs the host statement.  ``return_logprobs`` still reports the raw distribution.  Refused with ValueError, because a
    row could be left without a token: ``no_repeat_ngram_size`` > 0, ``min_new_tokens`` above the shortest sequence,
    ``suppress_tokens`` that meet the trie's tokens or the eos ids, a trie id >= V.  Not combined with beam search
    (NotImplementedError).  ``constraint=None`` is the call as it was.

    Classifier-free guidance (DESIGN.md "Classifier-free guidance"; greedy and sampled): ``guidance_scale`` != 1 with
    ``negative_embeddings`` asks every question twice -- under the prompt and under a negative prompt, e.g. the same text without
    its image (``Magma.embed_batch(batch, drop_images=True)``) -- and selects from u + guidance_scale * (c - u) over the two
    log_softmax distributions: the rule of transformers' ``guidance_scale`` / ``negative_prompt_ids``
    (``UnbatchedClassifierFreeGuidanceLogitsProcessor``; ``guide_logits`` above), the first processor of the chain, in front of the
    repetition penalty.  ``negative_embeddings`` takes what ``embeddings`` takes -- a (B, S', d) tensor, a (1, S', d) tensor that
    every row shares, a list of per-row tensors, embed_batch's (embeddings, lengths) -- with ``negative_lengths`` for the tensor
    forms; its length is independent of the prompt's.  ``guidance_min_p`` > 0 adds the plausibility cut of contrastive decoding:
    tokens less probable than guidance_min_p times the most probable one UNDER THE PROMPT are never selected.  The output is laid
    out as for the call on ``embeddings`` alone.  The HIP engine runs one cache of 2B ragged rows (the prompts, then the negative
    prompts), one prefill, and the token step over 2B rows with two small launches more (the combination in front of the
    processors, the token mirrored to the negative rows behind the bookkeeping); everything between them runs over B rows, so a
    guided row draws from the random stream of the same row unguided.  Any other LM object runs two model calls per step and the
    host statement.  ``return_logprobs`` still reports the raw conditional distribution.  ValueError: a scale that is negative or
    not finite, ``guidance_min_p`` outside [0, 1], a scale != 1 without a negative prompt, a negative prompt or ``guidance_min_p``
    at scale 1, row counts or hidden sizes that do not match.  Not combined with beam search, ``past_key_values`` or
    ``return_past_key_values`` (NotImplementedError): a guided cache holds two conversations per sample.  At the defaults the
    call is bit for bit what it was, and nothing is launched or allocated.

    Contrastive search (DESIGN.md "Contrastive search"; Su et al. 2022; ``penalty_alpha`` / ``top_k`` of transformers 4.x):
    ``penalty_alpha`` in (0, 1] with ``top_k`` in [1, 16] selects, among the ``top_k`` most probable next tokens, the one with the
    largest (1 - penalty_alpha) * p - penalty_alpha * (largest cosine of its hidden state -- the output of ln_f -- with the hidden
    state of any prompt position or earlier generated token): deterministic, and built for open-ended text such as captions,
    where greedy and beam search repeat themselves (``contrastive_search`` above; 0.6 and 4 are the paper's values).  ``top_k=0``
    with ``penalty_alpha`` > 0 is a ValueError.  ``temperature``, ``top_p``, ``seed`` and ``sampler`` do not apply, as with beam
    search.  Ragged prompts, ``decode``, ``stop_on_eos``, ``eos_check_every`` and the one-eos batch-wide stopping rule are greedy
    decoding's.  The HIP engine runs a cache of B * top_k rows -- every candidate is one row of the captured token step, whose
    weight stream they share -- with five small launches behind the head in place of the argmax and its bookkeeping; any other LM
    object runs the host statement on ``output_hidden_states``.  Not yet combined (NotImplementedError) with beam search /
    ``return_scores``, the logits processors, per-row stopping / several eos ids / ``return_finish``, ``return_logprobs``,
    ``constraint``, guidance, ``past_key_values`` / ``return_past_key_values``.  ``penalty_alpha=0.0`` (the default) is the call as
    it was, bit for bit, with the same launches and nothing allocated.

    Per-row sampling (DESIGN.md "Per-request sampling"; HIP engine only): ``seed``, ``temperature``, ``top_k``, ``top_p`` and
    ``min_p`` may each be a list, tuple or one-dimensional tensor of B values (a scalar stands for every row); any of them given so
    switches the call to the per-row mode.  Row b's j-th token (j = 0: the one selected from the prompt's logits) is then drawn
    from the Philox stream keyed by ITS seed at counter j, over ITS logits filtered by ITS settings -- the key and counter of the
    one-row call --, so for equal logits bits row b is the solo call ``generate(request_b, seed=seed_b, temperature=...,
    sampler=...)`` whatever its row and its neighbours are: n samples of one cached prompt (``cache_prompt`` +
    ``KVCache.expand(n)`` with n seeds) can each be regenerated alone, and greedy rows (temperature 0: the first maximum, no
    seed) sit beside sampled ones.  ``sampler`` stays one per call.  Every row is checked as the scalar call checks its arguments
    (ValueError names the row: a wrong length, ``min_p`` with the reference's sampler or on a greedy row, a value out of bounds);
    a sampled row without a seed draws one from torch's CPU generator.  Combines with ragged prompts, per-row stopping, the
    logits processors, log-probabilities, constraints, a continued cache and the quantised decode weights; not (NotImplementedError)
    with beam search, contrastive search or guidance.  The selection is the same single launch of the captured step, reading a
    device table (ops.sample_rows).  With scalars only, the call is what it was, bit for bit and launch for launch.

    Speculative decoding (DESIGN.md "Speculative decoding"; greedy at ``temperature=0.0``): ``prompt_lookup_num_tokens`` = k in
    [1, 7] makes every token step verify k guessed continuations per row beside the row's newest token -- k + 1 rows per
    sequence ride one weight stream -- and keep the longest prefix the model agrees with, plus the model's own next token: 1 to
    k + 1 tokens per step and row instead of one, token for token the output of ``generate(..., temperature=0.0,
    stop_per_row=True)``.  The guesses are transformers' prompt lookup (``prompt_lookup_num_tokens`` /
    ``max_matching_ngram_size`` there; ``prompt_lookup`` above): the continuation of the earliest earlier occurrence of the row's
    last ``max_matching_ngram_size`` (1 to 16; then fewer) tokens.  The prompt is embeddings, so its text is searched only when
    ``lookup_ids`` gives it: a list of B id lists, tensors or strings (``model.tokenizer.encode``), searched in front of the tokens
    this call generates; None searches those alone.  It pays where the answer repeats text that is there: few-shot answer formats,
    lists, OCR-like questions.  Speculation implies per-row stopping (``stop_per_row=None`` means True, False raises; ``eos_token``
    takes 1 to 8 ids; layout, padding and ``return_finish`` as there).  ``return_speculation=True`` appends a ``Speculation`` --
    per row the model calls it was open in, the drafts fed and the drafts accepted.  The HIP engine runs the whole step on the
    device (chunk attention, one bookkeeping launch that accepts, records and drafts again); any other LM object runs the host
    statement row by row.  B * (k + 1) may not exceed 16.  ``stop_sequences`` (HIP engine only) apply as in the plain call: every
    emitted token is tested, a draft that completes a sequence is accepted and the row finishes (``return_finish``: "stop" and
    the index).
    Sampled rows (HIP engine only; seed-exact, no rejection sampling): with ``temperature != 0`` or any of ``temperature``,
    ``top_k``, ``top_p``, ``min_p``, ``seed`` given per row, under either ``sampler``, the call ALWAYS selects by the per-row rule
    above -- scalars stand for every row, so ``seed=s`` means ``seed=[s] * B`` and ``None`` draws one seed per sampled row -- and
    fed position t of row b is drawn at the row's own counter (tokens emitted so far + t) under the row's own record: row b is,
    token for token, ``generate(row_b, ..., seed=s_b)`` alone, and the whole call is the plain per-row sampled call with
    ``stop_per_row=True``.  Greedy rows (temperature 0) may sit beside sampled ones.  An LM object without the engine is refused
    (``EngineOnlySpeculation``: a NotImplementedError and a ValueError), ``min_p`` on a greedy row too (ValueError).  Not yet combined (NotImplementedError) with beam and contrastive search,
    guidance, the logits processors, ``return_logprobs``, a constraint, ``past_key_values`` / ``return_past_key_values``,
    ``generate_stream`` / ``choose_stream``.  At ``prompt_lookup_num_tokens=0`` (the default) the call is launch for launch what
    it was."""
    if eos_token is None or (isinstance(eos_token, int) and not eos_token):
        eos_token = model.eos_token
    spec = check_speculation_args(prompt_lookup_num_tokens, max_matching_ngram_size, lookup_ids, return_speculation,
                                  vocab=_logit_count(model), encode=getattr(getattr(model, "tokenizer", None), "encode", None))
    if spec is not None:
        if stop_per_row is False:
            raise ValueError("speculative decoding (prompt_lookup_num_tokens > 0) stops per row: stop_per_row=False does not apply")
        stop_per_row = True
    per_row = per_row_given(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed)
    if per_row:
        for what, given in (("beam search (num_beams > 1 / return_scores=True)", num_beams > 1 or return_scores),
                            ("contrastive search (penalty_alpha > 0)", penalty_alpha != 0.0),
                            ("guidance (guidance_scale / negative_embeddings)", guidance_scale != 1.0 or negative_embeddings is not None)):
            if given:
                raise NotImplementedError(f"per-row sampler settings ({', '.join(per_row)} given per row) are not combined with {what}")
        # the scalar checks below see stand-ins for what is given per row; check_row_sampler_args checks every row once the
        # batch is known
        row_args = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed)
        stand_in = dict(temperature=1.0, top_k=0, top_p=0.9, min_p=0.0, seed=None)
        temperature, top_k, top_p, min_p, seed = (stand_in[k] if k in per_row else row_args[k] for k in ROW_SAMPLER_ARGS)
    early_stopping = check_beam_args(num_beams, num_return_sequences, early_stopping, num_beam_groups, diversity_penalty,
                                     _logit_count(model))
    proc = check_processor_args(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, _logit_count(model))
    stop = check_stop_args(eos_token, stop_sequences, stop_per_row, _logit_count(model),
                           getattr(getattr(model, "tokenizer", None), "encode", None))
    warp = check_sampler_args(sampler, min_p, top_p)
    if min_p > 0 and (num_beams > 1 or return_scores or temperature == 0.0):
        raise ValueError("min_p applies to sampled selection: greedy decoding (temperature=0) and beam search would drop it")
    if (stop is not None or return_finish) and (num_beams > 1 or return_scores):
        raise NotImplementedError("per-row stopping (a list of eos ids, stop_sequences, stop_per_row, return_finish) is not "
                                  "combined with beam search (num_beams > 1 / return_scores=True)")
    n_top = check_logprob_args(return_logprobs, top_logprobs, _logit_count(model))
    if n_top is not None and (num_beams > 1 or return_scores):
        raise NotImplementedError("token log-probabilities (return_logprobs / top_logprobs) are not combined with beam search "
                                  "(num_beams > 1 / return_scores=True): it has its own scores")
    eos_ids = stop["eos_ids"] if stop is not None else (eos_token,)
    eos_token = eos_ids[0]              # the pad id
    if constraint is not None and (num_beams > 1 or return_scores):
        raise NotImplementedError("a constraint is not combined with beam search (num_beams > 1 / return_scores=True): its "
                                  "candidate lists would fill with -inf entries")
    guide = check_guidance_args(guidance_scale, negative_embeddings, negative_lengths, guidance_min_p)
    if guide is not None and (num_beams > 1 or return_scores):
        raise NotImplementedError("guidance (guidance_scale / negative_embeddings) is not combined with beam search (num_beams > 1 "
                                  "/ return_scores=True): its running scores would mix two distributions")
    if guide is not None and (past_key_values is not None or return_past_key_values):
        raise NotImplementedError("guidance neither continues from nor returns a KV cache (past_key_values / "
                                  "return_past_key_values): a guided cache holds two conversations per row")
    continuing = past_key_values is not None or return_past_key_values
    contrast = check_contrastive_args(penalty_alpha, top_k, _logit_count(model))
    if spec is not None:
        for what, given in (("beam search (num_beams > 1 / return_scores=True) is", num_beams > 1 or return_scores),
                            ("contrastive search (penalty_alpha > 0) is", contrast is not None),
                            ("guidance is", guide is not None), ("the logits processors are", proc is not None),
                            ("token log-probabilities (return_logprobs / top_logprobs) are", n_top is not None),
                            ("a constraint is", constraint is not None),
                            ("a KV cache (past_key_values / return_past_key_values) is", continuing)):
            if given:
                raise NotImplementedError(f"{what} not combined with speculative decoding (prompt_lookup_num_tokens > 0) yet")
        # a sampled speculative call always selects by the per-row rule: scalars stand for every row (check_row_sampler_args, once
        # the batch is known).  temperature=0.0 as a scalar stays the greedy call, launch for launch.
        # A greedy call with stop sequences runs under the same rule with greedy records (the first maximum, mg_argmax_f32's token).
        sampled = None
        if per_row or temperature != 0.0 or stop["stop_seqs"]:
            sampled = dict(row_args if per_row else dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed),
                           sampler=sampler)
        return _generate_speculative(model, embeddings, lengths, max_steps, eos_ids, decode, eos_check_every, stop_on_eos, spec,
                                     lookup_ids, return_finish, return_speculation, stop["stop_seqs"], sampled)
    if contrast is not None:
        for what, given in (("beam search (num_beams > 1 / return_scores=True) is", num_beams > 1 or return_scores),
                            ("the logits processors are", proc is not None),
                            ("per-row stopping (a list of eos ids, stop_sequences, stop_per_row, return_finish) is",
                             stop is not None or return_finish),
                            ("token log-probabilities (return_logprobs / top_logprobs) are", n_top is not None),
                            ("a constraint is", constraint is not None), ("guidance is", guide is not None),
                            ("a KV cache (past_key_values / return_past_key_values) is", continuing)):
            if given:
                raise NotImplementedError(f"{what} not combined with contrastive search (penalty_alpha > 0) yet")
        if min_p > 0:
            raise ValueError("min_p applies to sampled selection: contrastive search (penalty_alpha > 0) would drop it")
        embeddings, lengths = prompt_batch(embeddings, lengths, check=False)
        return _generate_contrastive(model, embeddings, max_steps, eos_token, decode, eos_check_every, lengths, contrast[0],
                                     contrast[1], stop_on_eos)
    if continuing and (num_beams > 1 or return_scores):
        raise NotImplementedError("beam search neither continues from nor returns a KV cache (past_key_values / "
                                  "return_past_key_values need num_beams=1 and return_scores=False)")
    embeddings, lengths = prompt_batch(embeddings, lengths, check=False)
    # the HIP engine selects the token itself; any other LM object gets the reference's call (sampling.py:81-93)
    on_device = getattr(model.lm, "device_token_selection", False)
    if num_beams > 1 or return_scores:
        return _generate_beam(model, embeddings, max_steps, eos_token, decode, eos_check_every, lengths, num_beams,
                              float(length_penalty), early_stopping, num_return_sequences, return_scores, proc,
                              num_beam_groups, float(diversity_penalty))
    b, s, _ = embeddings.shape
    if per_row:
        row_records = check_row_sampler_args(b, sampler, **row_args)
        if not on_device:
            raise ValueError("per-row sampler settings need the HIP engine's LM (one selection launch reads every row's record)")
    if guide is not None:       # the negative prompt as (b, s', d) rows, row counts and hidden size checked
        guide = check_guidance_args(guidance_scale, negative_embeddings, negative_lengths, guidance_min_p, b, embeddings.shape[2])
    cons = check_constraint_args(constraint, b, getattr(getattr(model, "tokenizer", None), "encode", None), _logit_count(model),
                                 eos_ids, proc)
    if continuing and not on_device:
        raise ValueError("past_key_values / return_past_key_values need the HIP engine's LM")
    if continuing and max_steps < 1:
        raise ValueError("continuing a conversation needs max_steps >= 1")
    if past_key_values is not None and past_key_values.B != b:
        raise ValueError(f"the cache holds {past_key_values.B} rows, the new inputs {b}")
    lengths = prompt_batch(embeddings, lengths, per_row=on_device)[1]       # (the batch is normalised: this checks the lengths)
    if guide is not None and guide["lengths"] is not None and not on_device:
        raise ValueError("negative prompts of different lengths need the HIP engine's LM (per-row KV positions)")
    mode, seed = sampling_mode(temperature, top_k, top_p, warp, seed)
    if per_row:                 # ("rows", warp): the values travel in the cache's table, ``seed`` carries the rows' records to it
        mode, seed = ("rows", warp is not None), row_records
    modes = dict(mode=mode, proc=proc, stop=stop, n_top=n_top, cons=cons, guide=guide, eos_ids=eos_ids)
    want_finish = stop is not None and (return_finish or continuing or decode)      # the tail reads the per-row finish record
    with eval_mode(model):
        run = (_device_loop if on_device else _host_loop)(
            model, embeddings, lengths, max_steps, eos_token, seed, poll_every(eos_check_every), stop_on_eos, modes, want_finish,
            past_key_values)
        out, n_gen, past, record = run.out, run.out.shape[1] - s, run.past, run.record
        if record is None and return_finish:                              # the reference's rule: every row ran the whole call
            record = torch.tensor([[-1, 0]] * b).view(b, 2)
        finish = None if record is None else finish_from_record(record, n_gen)
        logprobs = None
        if n_top is not None:       # what the steps wrote (or the host statement's values), masked past every row's count
            vals = run.logprobs if n_gen else (torch.zeros(b, 0), torch.zeros(b, 0, n_top, dtype=torch.int64), torch.zeros(b, 0, n_top))
            logprobs = mask_logprobs(run.tokens, *vals, finish.kept if finish is not None else torch.full((b,), n_gen))
        if continuing:      # the cache keeps the conversation (a continued one too: it was advanced in place and stays continuable)
            keep_conversation(past, run.start, n_gen, eos_token, finish if stop is not None else None)
            model.lm.engine.detach_cache(past)
        if decode:          # per-row stopping: every row up to its own kept count
            out = decode_ids(model, out, eos_token, s, lengths, finish if stop is not None else None)
    ret = (out, past) if return_past_key_values else (out,)
    if return_finish:
        ret += (finish,)
    if n_top is not None:
        ret += (logprobs,)
    return ret if len(ret) > 1 else ret[0]


class _Generated(NamedTuple):
    """What a generate() loop hands to the shared tail: ``out`` (rows, s + n) ids laid out for the caller, ``tokens`` (rows, n) the
    generated columns, the LM's ``past``, the finish ``record`` (host [b, 2]; None when the tail does not read it), the per-step
    ``logprobs`` (lp, top ids, top lp; None without a step), ``start`` (engine: the cache position of every row's first new token),
    ``scores`` (engine, beam search: one per returned hypothesis)."""
    out: torch.Tensor
    tokens: torch.Tensor
    past: object = None
    record: Optional[torch.Tensor] = None
    logprobs: Optional[tuple] = None
    start: Optional[torch.Tensor] = None
    scores: Optional[torch.Tensor] = None


def _device_loop(model, embeddings, lengths, max_steps, eos_token, seed, every, stop_on_eos, modes, want_finish,
                 past_key_values, k: int = 1, first: bool = True, n_ret: int = 0) -> _Generated:
    """generate()'s loop on the HIP engine, in every selection mode: one prefill (or the new inputs appended to the caller's
    cache), then steps that feed the selected token back on the device -- nothing crosses the host but the all-eos step, read every
    ``every`` steps -- under ONE SelectionPlan built here from ``modes`` (generate()'s checked arguments by name; a missing one is
    None); the output is laid out from the token history the bookkeeping launch kept.  What beam and contrastive search change:
    ``k`` cache rows per sample (num_beams / top_k); ``first`` False: the prefill selects nothing, max_steps token steps follow
    it; ``n_ret`` > 0 (beam search): the poll always looks and cuts nothing, the tokens are beam_results(past, n_ret)."""
    from .engine import LMEngine
    b, s, _ = embeddings.shape
    dev = embeddings.device
    stop, n_top, guide = modes.get("stop"), modes.get("n_top"), modes.get("guide")
    plan = LMEngine.selection_plan(sampling=modes.get("mode"), beam=modes.get("beam"), processors=modes.get("proc"), stop=stop,
                                   logprobs=n_top, constraint=modes.get("cons"), contrast=modes.get("contrast"),
                                   guidance=None if guide is None else (guide["scale"], guide["min_p"]), vocab=model.lm.engine.V)
    if plan.is_rows:            # the rows' records as the host image of the device table (SelectionPlan._arm_first_token copies it)
        from . import ops
        seed = ops.sample_rows_table(*zip(*seed))
    first_kw = dict(eos_token=eos_token, seed=seed, plan=plan, lengths=lengths)
    own = lengths if lengths is not None else torch.full((b,), s, dtype=torch.int64)     # the positions every row adds
    prompts, start = embeddings, own
    if k > 1:                   # B prompts -> B * k rows, sample-major
        prompts = embeddings.repeat_interleave(k, dim=0)
        first_kw["lengths"] = None if lengths is None else lengths.repeat_interleave(k)
    if guide is not None:       # ONE ragged batch of 2b rows: the prompts, then the negative prompts
        neg = guide["embeddings"].to(device=dev, dtype=embeddings.dtype)
        s_neg = neg.shape[1]
        prompts = torch.zeros(2 * b, max(s, s_neg), embeddings.shape[2], dtype=embeddings.dtype, device=dev)
        prompts[:b, :s], prompts[b:, :s_neg] = embeddings, neg
        first_kw["lengths"] = torch.cat([own, guide["lengths"] if guide["lengths"] is not None
                                         else torch.full((b,), s_neg, dtype=torch.int64)])
    if past_key_values is not None:      # the new rows appended to the caller's cache (LMEngine.extend)
        before = past_key_values.rows_pos() + (past_key_values.pending >= 0).to(torch.int64) \
            if past_key_values.pending is not None else past_key_values.rows_pos()
        start, first_kw["lengths"] = before + own, own

    def prefill():              # into a pooled cache, or the new rows (``prompts`` are the embeddings) behind the caller's
        return model.lm(inputs_embeds=prompts, use_cache=True, past_key_values=past_key_values, cache_hint=max_steps,
                        reuse_cache=past_key_values is None, **first_kw)

    look = bool(n_ret) or (stop_on_eos and eos_token is not None)
    n_gen, past = 0, None if first else prefill().past_key_values
    for i in range(max_steps):
        if past is not None:    # the token selected by the previous step (or prefill) is fed back on the device
            outputs = model.lm(input_ids=None, use_cache=True, past_key_values=past, feed_back=True, plan=plan)
        else:
            outputs = prefill()
        past = outputs.past_key_values
        n_gen += 1
        if look and ((i + 1) % every == 0 or i + 1 == max_steps):
            all_eos = int(outputs.eos_state[1])          # one host sync per `every` steps
            if all_eos >= 0:
                n_gen = n_gen if n_ret else all_eos + 1  # tokens after the first all-eos step are dropped again
                break
    # (``[:b * k:k]``: a sample's k rows hold one history; a guided cache of 2b rows keeps the b guided rows' records first)
    tokens, scores = past.history[:b * k:k, :n_gen] if past is not None else torch.zeros(b, 0, dtype=torch.long, device=dev), None
    if n_ret:
        tokens, scores, _ = model.lm.engine.beam_results(past, n_ret)
    out = layout_ids(tokens.to(dev), s, lengths, model.image_token, eos_token, n_ret or 1)
    record = past.finish[:b].cpu() if stop is not None and (want_finish or (n_top is not None and n_gen)) else None
    vals = (past.lp[:b, :n_gen], past.top_id[:b, :n_gen], past.top_lp[:b, :n_gen]) if n_top is not None and n_gen else None
    return _Generated(out, tokens, past, record, vals, start, scores)


def _host_loop(model, embeddings, lengths, max_steps, eos_token, seed, every, stop_on_eos, modes, want_finish,
               past_key_values) -> _Generated:
    """generate()'s loop over any other LM object: the reference's call (sampling.py:81-93) and its host-side arithmetic, with
    the host statement of every mode in the engine's order -- guide_logits, process_logits, constrain_logits, the selection
    (warp_filter for transformers' sampler), token_logprobs of the raw row, stop_update.  (``lengths``, ``seed``, ``every`` and a
    cache belong to the engine's loop; generate() has refused ``lengths`` and a cache here.)"""
    b, s, _ = embeddings.shape
    dev = embeddings.device
    mode, proc, stop, n_top, cons, guide, eos_ids = (modes[k] for k in ("mode", "proc", "stop", "n_top", "cons", "guide", "eos_ids"))
    warp = mode is not None and mode[0] == "warp"
    temperature, top_k, top_p = mode[1:4] if warp else mode if mode is not None else (0.0, 0, 0.0)
    out = torch.full((b, s + max_steps), eos_token, dtype=torch.long, device=dev)
    out[:, :s] = model.image_token
    n, past = s, None
    host_lp = []                # per step (lp, top ids, top lp) of the host statement
    if stop is not None:
        done, record = torch.zeros(b, dtype=torch.bool), torch.tensor([[-1, 0]] * b, dtype=torch.int64).view(b, 2)
    for i in range(max_steps):
        if i == 0:
            outputs = model.lm(inputs_embeds=embeddings, use_cache=True, past_key_values=None, cache_hint=max_steps, reuse_cache=True)
        else:
            outputs = model.lm(input_ids=out[:, n - 1:n], use_cache=True, past_key_values=past)
        past = outputs.past_key_values
        logits = outputs.logits[:, -1, :].float()
        raw = logits
        if guide is not None:       # the negative stream: a second model call with its own past, then the host statement
            if i == 0:
                neg_out = model.lm(inputs_embeds=guide["embeddings"].to(dev), use_cache=True, past_key_values=None,
                                   cache_hint=max_steps)
            else:
                neg_out = model.lm(input_ids=out[:, n - 1:n], use_cache=True, past_key_values=neg_past)
            neg_past = neg_out.past_key_values
            logits = guide_logits(logits, neg_out.logits[:, -1, :].float(), guide["scale"], guide["min_p"]) \
                .to(torch.float32).to(logits.device)
        if proc is not None:
            logits = process_logits(logits.cpu(), out[:, s:n].cpu(), n - s, eos_token=eos_ids if stop is not None else eos_token,
                                    **proc).to(logits.device)
        if cons is not None:
            logits = constrain_logits(logits.cpu(), out[:, s:n].cpu(), n - s, cons, eos_ids).to(logits.device)
        if mode is None:
            next_token = outputs.next_token.unsqueeze(1) if outputs.get("next_token") is not None and proc is None \
                and cons is None and guide is None else \
                torch.argmax(logits, dim=-1, keepdim=True)
        else:
            if warp:
                logits = warp_filter(logits.cpu(), temperature, top_k, top_p, mode[4]).to(logits.device)
            if not warp and top_k > 0:
                logits = top_k_filter(logits, k=top_k)
            if not warp and top_p > 0:
                logits = top_p_filter(logits, threshold=top_p)
            probs = F.softmax(logits / temperature, dim=-1)
            next_token = torch.multinomial(probs, num_samples=1)
        if n_top is not None:       # of the raw distribution, for the token as selected (a finished row's is masked at the end)
            host_lp.append(token_logprobs(raw, next_token.view(-1), n_top))
        if stop is not None:        # the per-row rule (stop_update): finished rows are padded, the others tested
            next_token = torch.where(done.to(next_token.device)[:, None], torch.full_like(next_token, eos_token), next_token)
        out[:, n:n + 1] = next_token
        n += 1
        if stop is not None:
            was = done
            done, why = stop_update(out[:, s:n], n - s - 1, done, eos_ids, stop["stop_seqs"])
            now = done & ~was
            record[now, 0], record[now, 1] = n - s - 1, why[now, 0] * 256 + why[now, 1]
            if stop_on_eos and bool(done.all()):
                break
        elif stop_on_eos and eos_token is not None and bool((next_token == eos_token).all()):
            break
    n_gen = n - s
    vals = tuple(torch.stack([h[j] for h in host_lp[:n_gen]], 1) for j in range(3)) if n_top is not None and n_gen else None
    keep = stop is not None and (want_finish or (n_top is not None and n_gen))
    return _Generated(out[:, :n], out[:, s:n], past, record if keep else None, vals)


def _generate_speculative(model, embeddings, lengths, max_steps, eos_ids, decode, eos_check_every, stop_on_eos, spec, lookup_ids,
                          return_finish, return_speculation, stop_seqs=(), sampled=None):
    """generate() with prompt_lookup_num_tokens > 0: the checks that need the batch, the device or the host loop, and the
    per-row tail -- every row's tokens up to its own count, the pad id behind them.  ``sampled``: None (greedy), or
    check_row_sampler_args' keywords -- the rows' records then select on the HIP engine (("rows", warp))."""
    embeddings, lengths = prompt_batch(embeddings, lengths, check=False)
    b, s, _ = embeddings.shape
    on_device = getattr(model.lm, "device_token_selection", False)
    spec = check_speculation_args(spec["T"] - 1, spec["max_ngram"], lookup_ids, return_speculation, batch=b, vocab=_logit_count(model),
                                  encode=getattr(getattr(model, "tokenizer", None), "encode", None))
    if lengths is not None:
        from .engine import LMEngine
        lengths = LMEngine.check_lengths(lengths, b, s)
    pad = eos_ids[0]
    if sampled is not None:
        try:
            rows = check_row_sampler_args(b, **sampled)
        except ValueError as e:
            if "min_p applies" in str(e):       # a greedy row of the HIP engine's chunk selection takes its first maximum
                raise ValueError(f"{e} (the HIP engine's selection launch takes a greedy row's first maximum)") from None
            raise
        if not on_device:
            raise EngineOnlySpeculation(
                "speculative decoding (prompt_lookup_num_tokens > 0) of sampled rows (temperature != 0 or per-row sampler settings) "
                "and with stop sequences needs the HIP engine's LM: its selection launch draws every fed row at the sequence's own "
                "counter, its bookkeeping launch tests every emitted token; not combined with this LM object yet")
        spec = dict(spec, rows=rows, warp=sampled["sampler"] == "transformers")
    with eval_mode(model):
        loop = _speculate_device_loop if on_device else _speculate_host_loop
        history, count, record, stats = loop(model, embeddings, lengths, max_steps, eos_ids, poll_every(eos_check_every), spec,
                                             stop_seqs)
        n, n_gen = history.shape[1], int(count.max()) if stop_on_eos else max_steps
        tokens = torch.full((b, n_gen), pad, dtype=torch.int64)
        tokens[:, :n] = torch.where(torch.arange(n)[None, :] < count[:, None], history.cpu(), tokens[:, :n])
        out = layout_ids(tokens.to(embeddings.device), s, lengths, model.image_token, pad)
        finish = finish_from_record(record, n_gen)
        if decode:
            out = decode_ids(model, out, pad, s, lengths, finish)
    ret = (out,)
    if return_finish:
        ret += (finish,)
    if return_speculation:
        ret += (Speculation(stats[:, 0].clone(), stats[:, 1].clone(), stats[:, 2].clone()),)
    return ret if len(ret) > 1 else ret[0]


def _spec_record(finish) -> torch.Tensor:
    """The loop's finish record (count at which the row finished or -1, code) as finish_from_record reads one: a row that finished
    on an eos id or a stop sequence at count c did so at step c - 1; a row that ran out of its budget, or never finished, ran to the
    end of the call."""
    from .ops import STOP_EOS, STOP_SEQ
    rec = torch.as_tensor(finish).to(torch.int64).cpu().clone()
    eos = (rec[:, 0] >= 0) & (((rec[:, 1] & ~0xFF) == STOP_EOS) | ((rec[:, 1] & ~0xFF) == STOP_SEQ))
    rec[:, 0] = torch.where(eos, rec[:, 0] - 1, torch.full_like(rec[:, 0], -1))
    rec[:, 1] = torch.where(eos, rec[:, 1], torch.zeros_like(rec[:, 1]))
    return rec


def _speculate_device_loop(model, embeddings, lengths, max_steps, eos_ids, every, spec, stop_seqs=()):
    """The speculative loop on the HIP engine: one ragged prefill (every row keeps its own position: they advance by different
    amounts) armed with a speculative plan, then steps that feed their own ids back on the device; the host reads the
    all-finished latch every ``every`` steps, and once at the end the token history, the counts, the finish record and the
    statistics.  At most max_steps steps: every step emits at least one token per open row."""
    from .engine import LMEngine
    b, s, _ = embeddings.shape
    T = spec["T"]
    engine = model.lm.engine
    rows = spec.get("rows")
    plan = LMEngine.selection_plan(stop=dict(eos_ids=eos_ids, stop_seqs=stop_seqs), speculate=(T, spec["max_ngram"]), vocab=engine.V,
                                   sampling=None if rows is None else ("rows", spec["warp"]))
    arm = dict(limit=max_steps, lookup=spec["lookup"])
    if rows is not None:        # the sequences' records as the host image of the device table (_arm_speculate copies it)
        from . import ops
        arm["rows"] = ops.sample_rows_table(*zip(*rows))
    lens = lengths if lengths is not None else torch.full((b,), s, dtype=torch.int64)
    if max_steps < 1:
        return (torch.zeros(b, 0, dtype=torch.int64), torch.zeros(b, dtype=torch.int64), torch.tensor([[-1, 0]] * b).view(b, 2),
                torch.zeros(b, 3, dtype=torch.int64))
    outputs = model.lm(inputs_embeds=embeddings, use_cache=True, past_key_values=None, cache_hint=max_steps + T, reuse_cache=True,
                       eos_token=eos_ids[0], seed=arm, plan=plan, lengths=lens)
    past = outputs.past_key_values
    for i in range(max_steps - 1):
        outputs = model.lm(input_ids=None, use_cache=True, past_key_values=past, feed_back=True, plan=plan)
        if ((i + 1) % every == 0 or i + 2 == max_steps) and int(outputs.eos_state[1]) >= 0:     # one host sync per `every` steps
            break
    count, stats = engine.speculate_results(past, T)
    n = int(count.max())
    return past.history[:b, :n].cpu(), count, _spec_record(past.finish[:b]), stats


def _speculate_host_loop(model, embeddings, lengths, max_steps, eos_ids, every, spec, stop_seqs=()):
    """The speculative loop over any other LM object, the statement the device loop is compared with: row by row -- a row's
    prompt alone, then its last token and its drafts as ONE (1, 1 + drafts) chunk against its cache --, the greedy token of every
    fed position, speculate_update, and the cache cropped to the accepted length (crop_past)."""
    b, s, _ = embeddings.shape
    T, cols = spec["T"], max(max_steps, 1)
    rows = spec["lookup"] or [[] for _ in range(b)]
    width = max(len(q) for q in rows)
    st = dict(ids=torch.zeros(b, T, dtype=torch.int64), n_draft=torch.zeros(b, dtype=torch.int32),
              history=torch.zeros(b, cols, dtype=torch.int64), count=torch.zeros(b, dtype=torch.int32),
              finish=torch.tensor([[-1, 0]] * b, dtype=torch.int32).view(b, 2), pos=torch.zeros(b, dtype=torch.int32),
              stats=torch.zeros(b, 3, dtype=torch.int32), lookup=torch.zeros(b, width, dtype=torch.int32),
              lookup_len=torch.tensor([len(q) for q in rows], dtype=torch.int32), state=torch.tensor([0, -1], dtype=torch.int32))
    for r, q in enumerate(rows):
        st["lookup"][r, :len(q)] = torch.tensor(q, dtype=torch.int32)
    kw = dict(num_tokens=T - 1, max_ngram=spec["max_ngram"], eos_ids=eos_ids, limit=max_steps, vocab=_logit_count(model),
              stop_seqs=stop_seqs)

    def update(token, arm):
        speculate_update(st["ids"], st["n_draft"], token, st["history"], st["count"], st["finish"], st["pos"], st["stats"],
                         st["lookup"], st["lookup_len"], st["state"], arm=arm, **kw)

    if max_steps < 1:
        return st["history"][:, :0], st["count"].to(torch.int64), _spec_record(st["finish"]), st["stats"].to(torch.int64)
    pasts, token = [], torch.zeros(b, dtype=torch.int64)
    for r in range(b):
        n = s if lengths is None else int(lengths[r])
        out = model.lm(inputs_embeds=embeddings[r:r + 1, :n], use_cache=True, past_key_values=None, cache_hint=max_steps + T,
                       reuse_cache=False)
        pasts.append(out.past_key_values)
        token[r] = int(torch.argmax(out.logits[0, -1, :].float()))
        st["pos"][r] = n
    update(token, True)
    while int(st["state"][1]) < 0:
        token = torch.zeros(b * T, dtype=torch.int64)
        for r in range(b):
            if int(st["finish"][r, 0]) >= 0:
                continue
            fed = 1 + int(st["n_draft"][r])
            out = model.lm(input_ids=st["ids"][r:r + 1, :fed].to(embeddings.device), use_cache=True, past_key_values=pasts[r])
            pasts[r] = out.past_key_values
            token[r * T:r * T + fed] = torch.argmax(out.logits[0, -fed:, :].float(), dim=-1).cpu()
        update(token, False)
        for r in range(b):              # the rejected drafts leave the cache (a finished row's cache is not read again)
            if int(st["finish"][r, 0]) < 0:
                pasts[r] = crop_past(pasts[r], int(st["pos"][r]))
    n = int(st["count"].max())
    return st["history"][:, :n], st["count"].to(torch.int64), _spec_record(st["finish"]), st["stats"].to(torch.int64)


class StreamResult(NamedTuple):
    """One finished request of generate_stream()."""
    index: int                  # the request's ordinal in ``requests``
    tokens: torch.Tensor        # int64 CPU: the generated tokens that count, the finishing token included
    text: Optional[str]         # decoded as generate()'s per-row tail decodes (eos dropped, image tokens removed); None at decode=False
    reason: str                 # "eos" | "stop" | "length"
    reason_index: int           # which eos id / which stop sequence (-1 for "length")
    slot: Optional[int]         # the row of the session the request ran in (None: an LM object without slots)


class StreamRequest:
    """One request of ``generate_stream(..., per_request=True)`` with sampler settings and a seed of its own (DESIGN.md "Per-request
    sampling"): ``embeddings`` (1, S, d) / (S, d); a field left at None takes the session's keyword -- ``max_new_tokens``,
    ``temperature``, ``top_k``, ``top_p``, ``min_p``, and ``seed`` (the session's ``seed`` is the default seed of a request that gives
    none)."""
    __slots__ = ("embeddings", "max_new_tokens", "temperature", "top_k", "top_p", "min_p", "seed")

    def __init__(self, embeddings, max_new_tokens=None, temperature=None, top_k=None, top_p=None, min_p=None, seed=None):
        self.embeddings, self.max_new_tokens = embeddings, max_new_tokens
        self.temperature, self.top_k, self.top_p, self.min_p, self.seed = temperature, top_k, top_p, min_p, seed

    def __repr__(self):
        shape = tuple(self.embeddings.shape) if torch.is_tensor(self.embeddings) else type(self.embeddings).__name__
        return "StreamRequest(" + ", ".join([f"embeddings={shape}"] + [f"{k}={getattr(self, k)!r}" for k in self.__slots__[1:]
                                                                        if getattr(self, k) is not None]) + ")"


# what generate() takes and a request stream refuses when it differs from generate()'s default
_STREAM_REFUSED = (
    ("the logits processors are", ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")),
    ("token log-probabilities (return_logprobs / top_logprobs) are", ("return_logprobs", "top_logprobs")),
    ("a constraint is", ("constraint",)),
    ("guidance is", ("guidance_scale", "negative_embeddings", "negative_lengths", "guidance_min_p")),
    ("beam search is", ("num_beams", "num_beam_groups", "diversity_penalty", "length_penalty", "early_stopping",
                        "num_return_sequences", "return_scores")),
    ("contrastive search is", ("penalty_alpha",)),
    ("a KV cache (past_key_values / return_past_key_values) is", ("past_key_values", "return_past_key_values")),
    ("speculative decoding is", ("prompt_lookup_num_tokens", "max_matching_ngram_size", "lookup_ids", "return_speculation")),
)


def _max_positions(model):
    cfg = getattr(getattr(model, "lm", None), "config", None)
    n = getattr(cfg, "max_position_embeddings", None) or getattr(cfg, "n_positions", None)
    return int(n) if isinstance(n, int) else None


def _stream_args(model, slots, max_new_tokens, max_prompt, every, admit_rows, prefix, share_prefix, budget="max_new_tokens"):
    """The session arguments generate_stream and choose_stream share, checked when the call is made: returns (on_device,
    admit_rows, every, prefix as (P, d) embeddings or a KVCache or None, P, max_prompt).  ``budget``: what the caller names
    ``max_new_tokens`` in its messages."""
    on_device = getattr(model.lm, "device_token_selection", False)
    for name, v, lo, hi in (("slots", slots, 1, 16), (budget, max_new_tokens, 1, None)):
        if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"{name} must be an integer in [{lo}, {hi if hi is not None else '...'}], got {v!r}")
    if admit_rows is None:
        admit_rows = slots
    if isinstance(admit_rows, bool) or not isinstance(admit_rows, int) or not 1 <= admit_rows <= slots:
        raise ValueError(f"admit_rows must be an integer in [1, slots = {slots}], got {admit_rows!r}")
    if every is None:
        every = poll_every()
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"every must be an integer >= 1, got {every!r}")
    n_pos = _max_positions(model)
    P = 0
    if not isinstance(share_prefix, bool):
        raise ValueError(f"share_prefix must be True or False, got {share_prefix!r}")
    if share_prefix and prefix is None:
        raise ValueError("share_prefix=True needs a prefix: there is nothing to share")
    if prefix is not None:
        if torch.is_tensor(prefix):
            if prefix.ndim not in (2, 3) or (prefix.ndim == 3 and prefix.shape[0] != 1) or prefix.shape[-2] < 1:
                raise ValueError(f"prefix must be embeddings (P, d) or (1, P, d) with P >= 1, or a one-row KVCache, got "
                                 f"{tuple(prefix.shape)}")
            prefix = prefix[0] if prefix.ndim == 3 else prefix
            cfg = getattr(model.lm, "config", None)
            width = getattr(cfg, "hidden_size", None) or getattr(cfg, "n_embd", None)
            if isinstance(width, int) and prefix.shape[1] != width:
                raise ValueError(f"prefix must be embeddings of width {width}, got {tuple(prefix.shape)}")
            P = prefix.shape[0]
        elif type(prefix).__name__ != "KVCache":
            raise ValueError(f"prefix must be embeddings (P, d) or (1, P, d), or a one-row KVCache, got {type(prefix).__name__}")
        elif not on_device:
            raise ValueError("a KVCache prefix needs the HIP engine's LM: pass the prefix's embeddings")
        if on_device:           # the session's own checks, now: the cache's rows, pending token, kind and engine, the width
            from .engine import SlotSession
            P = SlotSession.prefix_rows(model.lm.engine, prefix)
    before = f"a prefix of {P} rows + " if P else ""
    if max_prompt is None:
        if n_pos is None:
            raise ValueError("max_prompt is needed: this LM object does not say its max_position_embeddings")
        max_prompt = (n_pos - P - max_new_tokens) // 64 * 64
        if max_prompt < 1:
            raise ValueError(f"{before}{budget} = {max_new_tokens} leaves no room for a prompt within max_position_embeddings = "
                             f"{n_pos}; pass max_prompt")
    if isinstance(max_prompt, bool) or not isinstance(max_prompt, int) or max_prompt < 1:
        raise ValueError(f"max_prompt must be an integer >= 1, got {max_prompt!r}")
    if n_pos is not None and P + max_prompt + max_new_tokens > n_pos:
        raise ValueError(f"{before}max_prompt = {max_prompt} + {budget} = {max_new_tokens} exceeds max_position_embeddings = {n_pos}")
    if n_pos is not None and P and on_device and P + (max_prompt + 63) // 64 * 64 > n_pos:
        raise ValueError(f"{before}max_prompt = {max_prompt}, staged as {(max_prompt + 63) // 64 * 64} rows, exceeds "
                         f"max_position_embeddings = {n_pos}")
    return on_device, admit_rows, every, prefix, P, max_prompt


def generate_stream(model, requests, *, slots: int = 8, max_new_tokens: int = 100, max_prompt: int = None, eos_token=None,
                    stop_sequences=None, temperature: float = 0.0, top_k: int = 0, top_p: float = 0.9,
                    sampler: str = "reference", min_p: float = 0.0, seed: int = None, every: int = None, admit_rows: int = None,
                    decode: bool = True, prefix=None, share_prefix: bool = False, per_request: bool = False, **unsupported):
    """Generate over a stream of requests (DESIGN.md "Request streams"): yields one ``StreamResult`` per request, in completion
    order.  Request i's tokens, finish reason and index are those of the solo call

        generate(model, request_i, max_steps=max_new_tokens_i, eos_token=[...], stop_sequences=..., stop_per_row=True,
                 return_finish=True, temperature=0.0)

    -- that call is the host statement, and for an LM object that is not the HIP engine exactly those calls run one after
    another.  The HIP engine runs a slot session (engine.SlotSession): ``slots`` rows (1 to 16, the range of the captured GEMV step)
    generate in one captured token step, and the row of a finished request goes to the next request while the others keep
    generating; nothing of the token step changes but its bookkeeping launch (ops.sample_finish_slots).

    ``requests``: any iterable of embeddings tensors (1, S, d) / (S, d), as ``embed`` returns them, or pairs (embeddings,
    max_new_tokens_i) with 1 <= max_new_tokens_i <= ``max_new_tokens`` (the default budget and the session's bound).  It is pulled
    lazily, one item when a slot frees, so a data loader or preprocess_inputs + embed can run inside it on the same stream.
    ``max_prompt``: the longest prompt the session takes (default: max_position_embeddings - max_new_tokens rounded down to 64).
    It sets the cost of the session: EVERY admission prefill runs over (admit_rows, ceil64(max_prompt)) rows whatever the real
    prompt lengths are, and the session allocates a live cache of ``slots`` x ceil64(max_prompt + max_new_tokens) positions plus a
    staging cache of admit_rows x ceil64(max_prompt) -- at the default, 28 blocks and 8 slots about 15 GB and prefills of 1920
    rows per row: pass the longest prompt you expect.  A longer prompt (or any other bad item) raises ValueError naming the
    request when it is pulled: nothing more is pulled, the requests in front of it are generated to their end and yielded
    first, then the error is raised -- no earlier request is lost, and the engine stays usable.
    ``every``: the number of steps between two host looks (default MAGMA_EOS_CHECK_EVERY, as generate).  ``admit_rows`` (1 to
    ``slots``, default ``slots``): the fixed row count of every admission prefill -- the staging shape (admit_rows,
    ceil64(max_prompt)) is fixed for the session so that a request's bits do not depend on what was admitted with it.
    ``eos_token`` (an id or 1 to 8 ids; default the model's) and ``stop_sequences`` are generate()'s per-row stopping arguments.
    Greedy decoding (``temperature=0``, the default) and both samplers are supported.  A sampled request draws its first token
    at its admission from the Philox counter (2^32 - 1 - admission pass, staging row) and every later token from (global step
    of the session, slot) -- two domains that never meet, so no two draws of a session share a counter (engine.SlotSession) --,
    NOT from the counters of a solo call: in this session-wide mode only greedy decoding and ``top_k=1`` are reproducible against a
    solo call.
    ``per_request=True`` (DESIGN.md "Per-request sampling"): every request has sampler settings and a seed of its own, and a sampled
    request IS reproducible against its solo call.  An item may then also be a ``StreamRequest(embeddings, max_new_tokens=None,
    temperature=None, top_k=None, top_p=None, min_p=None, seed=None)``; a field left at None -- and every field of a plain tensor or
    pair item -- takes the session's keyword, the session's ``seed`` being the default seed of a request that gives none (a sampled
    request without either draws one from torch's CPU generator when it is pulled).  Request i's tokens, reason and index are
    those of the solo call above with ``temperature=, top_k=, top_p=, min_p=, seed=`` of request i and the session's ``sampler``
    (the rule set stays one per session): its j-th token is drawn from the Philox stream keyed by ITS seed at counter j over ITS
    logits filtered by ITS settings, the first at its admission, so its tokens do not depend on its slot, on the requests beside
    it, on ``every``, on ``admit_rows`` or on the admission pass, and greedy and sampled requests share a session.  The HIP engine
    reads the settings from a device table inside the same selection launch of the same captured step (ops.sample_rows); an LM
    object that is not the HIP engine runs the solo calls one after another with each request's own settings.  A
    ``StreamRequest`` without ``per_request=True`` raises ValueError when it is pulled.  With ``per_request=False`` (the default)
    everything is what it was.  Not combined (NotImplementedError): the logits processors, return_logprobs, constraint,
    guidance, beam and contrastive search, past_key_values.  (A closed answer set per request with its log-probabilities and the
    rules is ``choose_stream``, whose session runs the constraint, rule and log-probability kernels over the ring.)
    The arguments are checked when the call is made; the work starts with the first ``next``.
    ``prefix`` (DESIGN.md "Request streams", session prefix): ONE prompt in front of every request -- the few-shot exemplars of an
    evaluation --, as (P, d) / (1, P, d) embeddings or as a one-row KVCache from ``Magma.cache_prompt`` (HIP engine only; only
    read: its K / V, positions and pending token are what they were after the session, other calls may keep expanding and
    continuing it).  Request i's tokens, reason and index are then those of the solo call above on ``request_i`` with
    ``past_key_values=<a private copy of the prefix cache>``; an LM object that is not the HIP engine runs the solo calls on
    ``torch.cat([prefix, request_i])``.  The prefix is prefilled ONCE and copied into every slot and every staging row at set-up;
    an admission prefill still runs over (admit_rows, ceil64(max_prompt)) rows -- the requests' own rows, appended behind the
    cached prefix --, not over (admit_rows, ceil64(P + max_prompt)).  ``max_prompt`` keeps its meaning, the longest request NOT
    counting the prefix; its default becomes (max_position_embeddings - P - max_new_tokens) rounded down to 64, and
    P + max_prompt + max_new_tokens (and the staged P + ceil64(max_prompt)) must fit max_position_embeddings.  Memory: a live
    cache of ``slots`` x ceil64(P + max_prompt + max_new_tokens) positions plus a staging cache of admit_rows x
    (P + ceil64(max_prompt)).  Every slot holds its OWN copy of the prefix, so the decode attention of a token step reads P more
    positions per live row: a prefix saves prefill work, not decode bandwidth.  ValueError at call time: a cache with several
    rows, with a pending token, of a beam or contrastive search or of another engine, embeddings of the wrong width.
    ``share_prefix=True`` (DESIGN.md "Shared session prefix"; needs ``prefix``, ValueError at call time without one): the session
    keeps ONE copy of the prefix's K / V and the live cache holds the rows' own positions only -- ``slots`` x
    ceil64(max_prompt + max_new_tokens).  The decode attention of a token step then reads the prefix once for all rows (one launch
    per block computes every row's partial attention over it, cut into chunks that depend on P alone; the attention launch merges
    them with the row's own keys).  The sums are formed in another order than in the per-slot copies' attention, so tokens agree
    with the default up to near-ties; a request's tokens do not depend on its slot, on the other requests or on ``every``.  An
    LM object that is not the HIP engine ignores the flag."""
    import inspect
    defaults = {k: p.default for k, p in inspect.signature(generate).parameters.items()}
    known = {k for _, names in _STREAM_REFUSED for k in names}
    for k in unsupported:
        if k not in known:
            raise TypeError(f"generate_stream() got an unexpected keyword argument {k!r}")
    for what, names in _STREAM_REFUSED:
        for k in names:
            if k in unsupported and not (unsupported[k] is defaults[k] or (not torch.is_tensor(unsupported[k]) and unsupported[k] == defaults[k])):
                raise NotImplementedError(f"{what} not combined with generate_stream yet ({k}=)")
    on_device, admit_rows, every, prefix, P, max_prompt = _stream_args(model, slots, max_new_tokens, max_prompt, every, admit_rows,
                                                                       prefix, share_prefix)
    if eos_token is None or (isinstance(eos_token, int) and not isinstance(eos_token, bool) and not eos_token):
        eos_token = model.eos_token
    stop = check_stop_args(eos_token, stop_sequences, True, _logit_count(model),
                           getattr(getattr(model, "tokenizer", None), "encode", None))
    warp = check_sampler_args(sampler, min_p, top_p)
    if not isinstance(per_request, bool):
        raise ValueError(f"per_request must be True or False, got {per_request!r}")
    if min_p > 0 and temperature == 0.0 and not per_request:
        raise ValueError("min_p applies to sampled selection: greedy decoding (temperature=0) would drop it")
    if per_request:             # the values travel with the requests; the session's are the defaults of their None fields
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError(f"seed must be an integer or None, got {seed!r}")
        mode = ("rows", warp is not None)
        session_values = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed)
    else:
        mode, seed = sampling_mode(temperature, top_k, top_p, warp, seed)

    def record_of(index, item):
        """Request ``index``'s (temperature, top_k, top_p, min_p, seed), checked as generate() checks a row's."""
        given = {k: getattr(item, k, None) for k in ROW_SAMPLER_ARGS}
        try:
            return check_row_sampler_args(1, sampler, **{k: session_values[k] if v is None else v for k, v in given.items()})[0]
        except ValueError as e:
            raise ValueError(f"request {index}: {str(e).replace('row 0: ', '', 1)}") from None

    def pulled():
        """(index, (S, d) embeddings, limit) of every request, checked as it is pulled -- with ``per_request``, followed by the
        request's record (temperature, top_k, top_p, min_p, seed)."""
        for index, item in enumerate(requests):
            if isinstance(item, StreamRequest):
                if not per_request:
                    raise ValueError(f"request {index}: a StreamRequest needs generate_stream(..., per_request=True)")
                emb, limit = item.embeddings, max_new_tokens if item.max_new_tokens is None else item.max_new_tokens
            else:
                emb, limit = item if isinstance(item, (tuple, list)) else (item, max_new_tokens)
            if not torch.is_tensor(emb) or emb.ndim not in (2, 3) or (emb.ndim == 3 and emb.shape[0] != 1):
                raise ValueError(f"request {index}: an item is an embeddings tensor (1, S, d) or (S, d), or a pair of one and its "
                                 "max_new_tokens")
            emb = emb[0] if emb.ndim == 3 else emb
            if isinstance(limit, bool) or not isinstance(limit, int) or not 1 <= limit <= max_new_tokens:
                raise ValueError(f"request {index}: max_new_tokens must be an integer in [1, {max_new_tokens}] (the session's "
                                 f"max_new_tokens), got {limit!r}")
            if not 1 <= emb.shape[0] <= max_prompt:
                raise ValueError(f"request {index}: a prompt of {emb.shape[0]} rows is outside [1, max_prompt = {max_prompt}]")
            if per_request:
                yield index, emb, limit, record_of(index, item)
            else:
                yield index, emb, limit

    def text_of(ids, reason):
        if not decode:
            return None
        ids = ids.tolist()[:-1] if reason == "eos" else ids.tolist()
        return model.tokenizer.decode([t for t in ids if t != model.image_token])

    def solo_calls():           # the host statement, request after request
        kw = dict(eos_token=list(stop["eos_ids"]), stop_sequences=[list(q) for q in stop["stop_seqs"]] or None, stop_per_row=True,
                  return_finish=True, decode=False, temperature=temperature, top_k=top_k, top_p=top_p, sampler=sampler, min_p=min_p,
                  seed=seed, eos_check_every=every)
        for index, emb, limit, *record in pulled():
            if P:
                emb = torch.cat([prefix.to(emb.device, emb.dtype), emb])
            if record:          # per_request: the request's own settings and seed reach its solo call
                kw.update(zip(ROW_SAMPLER_ARGS, record[0]))
            out, fin = generate(model, emb[None], max_steps=limit, **kw)
            ids = out[0, emb.shape[0]: emb.shape[0] + int(fin.kept[0])].to("cpu", torch.int64)
            yield StreamResult(index, ids, text_of(ids, fin.reason[0]), fin.reason[0], fin.index[0], None)

    def session():
        from .engine import LMEngine, SlotSession
        eng = model.lm.engine
        if getattr(model, "device", None) is not None and torch.device(model.device).type == "cuda":
            torch.cuda.set_device(model.device)
        plan = LMEngine.selection_plan(sampling=mode, stop=stop, vocab=eng.V, slots=True)
        ses = SlotSession(eng, plan, slots=slots, max_new=max_new_tokens, max_prompt=max_prompt, every=every,
                          admit_rows=admit_rows, seed=None if per_request else seed, prefix=prefix, share_prefix=share_prefix)
        dev = eng.device
        for index, ids, code, slot in ses.run((i, e.to(dev), n, *rest) for i, e, n, *rest in pulled()):
            reason = REASON_NAMES[code >> 8]
            yield StreamResult(index, ids, text_of(ids, reason), reason, -1 if reason == "length" else code & 255, slot)

    return session() if on_device else solo_calls()


def choose(model, embeddings, choices, lengths=None, **generate_kwargs):
    """Which of ``choices`` the model answers with (Magma.choose): constrained greedy decoding with ``return_logprobs=True`` and
    ``max_steps`` = the longest choice + 1, every row's tokens mapped back with ``TokenTrie.index``.  ``choices``: what
    ``generate(constraint=...)`` takes.  Returns (index int64 [B] -- the position of the row's answer in its list of choices --,
    TokenLogprobs of the path under the raw distribution; ``count[b]`` = the answer's tokens + the eos that ended it).
    Rows stop on their own (``stop_per_row=True`` unless given).  It follows the GREEDY path through the trie: the most probable
    next token among those allowed, step by step.  It is NOT the arg-max of the total sequence probability -- a choice whose
    first token is unlikely loses even if the rest of it is certain; ``rank`` below gives every choice's total in one forward."""
    fixed = {"max_steps", "temperature", "decode", "constraint", "return_logprobs", "return_finish", "return_past_key_values",
             "num_beams", "return_scores"} & set(generate_kwargs)
    if fixed:
        raise ValueError(f"choose() sets {sorted(fixed)} itself")
    embeddings, lengths = prompt_batch(embeddings, lengths, check=False)
    b = embeddings.shape[0]
    tries = check_constraint_args(choices, b, getattr(getattr(model, "tokenizer", None), "encode", None), _logit_count(model))
    if tries is None:
        raise ValueError("choose() needs choices")
    generate_kwargs.setdefault("stop_per_row", True)
    _, lp = generate(model, embeddings, max_steps=max(t.max_len() for t in tries) + 1, temperature=0.0, decode=False,
                     lengths=lengths, constraint=tries, return_logprobs=True, **generate_kwargs)
    eos = generate_kwargs.get("eos_token")
    if eos is None or (isinstance(eos, int) and not eos):
        eos = model.eos_token
    eos = set(eos.tolist() if torch.is_tensor(eos) else eos if isinstance(eos, (list, tuple)) else [eos])
    index = torch.full((b,), -1, dtype=torch.int64)
    for r in range(b):
        ids = lp.tokens[r, : int(lp.count[r])].tolist()
        while ids and ids[-1] in eos:
            ids.pop()
        index[r] = tries[r].index(ids)
    return index, lp


class StreamChoice(NamedTuple):
    """One finished request of choose_stream(): CPU tensors over the answer's ``count`` tokens."""
    index: int                  # the request's ordinal in ``requests``
    choice: int                 # the position of the answer in the request's list of choices
    tokens: torch.Tensor        # int64 [count]: the answer's tokens and the eos that ended it
    logprobs: torch.Tensor      # fp32 [count]: log p(tokens[i]) under the raw model distribution of that step
    top_ids: torch.Tensor       # int64 [count, top_logprobs]
    top_logprobs: torch.Tensor  # fp32 [count, top_logprobs]
    reason: str                 # "eos" (a walk through a trie always ends there within its budget) | "length"
    slot: Optional[int]         # the row of the session the request ran in (None: an LM object without slots)


def choose_stream(model, requests, *, slots: int = 8, max_choice_tokens: int = 16, max_prompt: int = None, eos_token=None,
                  top_logprobs: int = 0, every: int = None, admit_rows: int = None, prefix=None, share_prefix: bool = False,
                  trie_capacity: int = None, repetition_penalty: float = 1.0, min_new_tokens: int = 0, suppress_tokens=None,
                  **unsupported):
    """``choose`` over a stream of requests (DESIGN.md "Choosing over a request stream"): every request brings its own closed set
    of answers, and one ``StreamChoice`` per request is yielded in completion order.  Request i's choice, tokens and
    log-probabilities are those of the solo call

        choose(model, request_i, choices_i, eos_token=..., top_logprobs=..., [past_key_values=<a private copy of the prefix cache>],
               repetition_penalty=..., min_new_tokens=..., suppress_tokens=...)

    -- that call is the definition, and for an LM object that is not the HIP engine exactly those calls run one after another (on
    ``torch.cat([prefix, request_i])`` with a prefix).  The HIP engine runs generate_stream's slot session under a plan with the
    constraint, the rules and the log-probabilities: a short answer frees its row for the next request while longer ones go on.

    ``requests``: any iterable of pairs (embeddings (1, S, d) / (S, d), choices); ``choices`` is what ``choose`` takes for ONE row:
    a ``TokenTrie``, or a list of id sequences or strings.  Requests that pass the same TokenTrie OBJECT share its entry in the
    device table; a list is built into a trie of its own when the request is pulled.  The request's budget is its longest choice
    + 1 (the eos); ``max_choice_tokens`` (1 to 64) bounds every choice of the session.  A request is checked when it is pulled,
    under generate_stream's rule: bad choices, or a choice longer than ``max_choice_tokens``, raise ValueError naming the request
    after the requests in front of it were finished and yielded.  Selection is greedy, as in ``choose``.
    ``slots``, ``max_prompt``, ``every``, ``admit_rows``, ``prefix``, ``share_prefix``, ``eos_token`` (an id or 1 to 8 ids): as in
    generate_stream, with max_choice_tokens + 1 as the session's token budget.  ``top_logprobs``: the alternatives per token.
    ``trie_capacity``: int32 entries the device table is allocated for (3 + 4 nodes + 2 edges, summed over the tries that are live
    at once; default 4096) -- a table that outgrows it is re-allocated mid-session, and the captured step with it.
    ``repetition_penalty`` / ``min_new_tokens`` / ``suppress_tokens``: generate()'s rules, checked against every request's choices
    as generate(constraint=...) checks them.  generate()'s speculation keywords are refused (NotImplementedError) when they differ
    from their defaults, as generate_stream refuses them."""
    import inspect
    defaults = {k: p.default for k, p in inspect.signature(generate).parameters.items()}
    spec_names = _STREAM_REFUSED[-1][1]
    for k, v in unsupported.items():
        if k not in spec_names:
            raise TypeError(f"choose_stream() got an unexpected keyword argument {k!r}")
        if not (v is defaults[k] or (not torch.is_tensor(v) and v == defaults[k])):
            raise NotImplementedError(f"speculative decoding is not combined with choose_stream yet ({k}=)")
    for name, v, lo, hi in (("max_choice_tokens", max_choice_tokens, 1, MAX_TRIE_LEN), ("trie_capacity", trie_capacity, 1, None)):
        if (name != "trie_capacity" or v is not None) and (isinstance(v, bool) or not isinstance(v, int) or v < lo or
                                                          (hi is not None and v > hi)):
            raise ValueError(f"{name} must be an integer in [{lo}, {hi if hi is not None else '...'}], got {v!r}")
    budget = max_choice_tokens + 1
    on_device, admit_rows, every, prefix, P, max_prompt = _stream_args(model, slots, budget, max_prompt, every, admit_rows, prefix,
                                                                       share_prefix, budget="max_choice_tokens + 1")
    V = _logit_count(model)
    encode = getattr(getattr(model, "tokenizer", None), "encode", None)
    if eos_token is None or (isinstance(eos_token, int) and not isinstance(eos_token, bool) and not eos_token):
        eos_token = model.eos_token
    stop = check_stop_args(eos_token, None, True, V, encode)
    eos_ids = [int(t) for t in stop["eos_ids"]]
    n_top = check_logprob_args(True, top_logprobs, V)
    rules = dict(repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens)
    proc = check_processor_args(vocab=V, **rules)

    def pulled():
        """(index, (S, d) embeddings, TokenTrie) of every request, checked as it is pulled."""
        for index, item in enumerate(requests):
            if not isinstance(item, (tuple, list)) or len(item) != 2:
                raise ValueError(f"request {index}: an item is a pair (embeddings, choices)")
            emb, choices = item
            if not torch.is_tensor(emb) or emb.ndim not in (2, 3) or (emb.ndim == 3 and emb.shape[0] != 1):
                raise ValueError(f"request {index}: the embeddings are a tensor (1, S, d) or (S, d)")
            emb = emb[0] if emb.ndim == 3 else emb
            if not 1 <= emb.shape[0] <= max_prompt:
                raise ValueError(f"request {index}: a prompt of {emb.shape[0]} rows is outside [1, max_prompt = {max_prompt}]")
            try:
                trie = (check_constraint_args(choices, 1, encode, V, eos_ids, proc) or [None])[0]
            except ValueError as e:
                raise ValueError(f"request {index}: {e}") from None
            if trie is None:
                raise ValueError(f"request {index}: choose_stream needs choices")
            if trie.max_len() > max_choice_tokens:
                raise ValueError(f"request {index}: a choice of {trie.max_len()} tokens exceeds max_choice_tokens = {max_choice_tokens}")
            yield index, emb, trie

    def result(index, trie, ids, lp, top_ids, top_lp, slot):
        ids = ids.to("cpu", torch.int64)
        answer = ids.tolist()
        reason = "eos" if answer and answer[-1] in eos_ids else "length"
        while answer and answer[-1] in eos_ids:
            answer.pop()
        return StreamChoice(index, trie.index(answer), ids, lp, top_ids, top_lp, reason, slot)

    def solo_calls():           # the definition, request after request
        for index, emb, trie in pulled():
            if P:
                emb = torch.cat([prefix.to(emb.device, emb.dtype), emb])
            _, lp = choose(model, emb[None], trie, eos_token=list(eos_ids), top_logprobs=n_top, eos_check_every=every, **rules)
            n = int(lp.count[0])
            yield result(index, trie, lp.tokens[0, :n], lp.logprobs[0, :n], lp.top_ids[0, :n], lp.top_logprobs[0, :n], None)

    def session():
        from .engine import LMEngine, SlotSession
        eng = model.lm.engine
        if getattr(model, "device", None) is not None and torch.device(model.device).type == "cuda":
            torch.cuda.set_device(model.device)
        plan = LMEngine.selection_plan(stop=stop, processors=None if proc is None else rules, logprobs=n_top, constraint=True,
                                       vocab=eng.V, slots=True)
        ses = SlotSession(eng, plan, slots=slots, max_new=budget, max_prompt=max_prompt, every=every, admit_rows=admit_rows,
                          prefix=prefix, share_prefix=share_prefix, trie_capacity=trie_capacity)
        dev, tries = eng.device, {}

        def items():
            for index, emb, trie in pulled():
                tries[index] = trie
                yield index, emb.to(dev), trie.max_len() + 1, trie

        for index, ids, _, slot, (lp, top_ids, top_lp) in ses.run(items()):
            yield result(index, tries.pop(index), ids, lp, top_ids, top_lp, slot)

    return session() if on_device else solo_calls()


class Ranking(NamedTuple):
    """What rank() returns: CPU tensors over the B rows and the C = most choices of a row, in the caller's order; a row with fewer
    choices is padded with -inf / 0."""
    index: torch.Tensor         # int64 [B]: the arg-max of scores, the lowest position on an exact tie
    scores: torch.Tensor        # fp32 [B, C]: logprobs / count ** length_penalty
    logprobs: torch.Tensor      # fp32 [B, C]: sum_j log p(choice[j] | prompt, choice[:j]) (+ log p(eos | prompt, choice))
    count: torch.Tensor         # int64 [B, C]: the number of terms


def rank_groups(trie: TokenTrie, budget: int) -> List[List[int]]:
    """The listed sequences of ``trie`` (positions of its list) in groups whose tries hold at most ``budget`` nodes each: whole
    sequences, consecutive in preorder (lexicographic order), so the first group's nodes keep the rows they have in the whole trie;
    a duplicate stays with its first copy.  One group when everything fits.  ValueError when one sequence alone does not."""
    at = {}
    for c, q in enumerate(trie.sequences):
        at.setdefault(q, []).append(c)
    groups, cur, n, prev = [], [], 0, ()
    for q in sorted(at):
        if len(q) > budget:
            raise ValueError(f"a choice of {len(q)} tokens does not fit into {budget} free positions")
        keep = 0
        while cur and keep < min(len(prev), len(q)) and prev[keep] == q[keep]:
            keep += 1
        if cur and n + len(q) - keep > budget:
            groups.append(cur)
            cur, n, keep = [], 0, 0
        cur = cur + at[q]
        n += len(q) - keep
        prev = q
    groups.append(cur)
    return groups


def _rank_host(model, embeddings, lens, tries, eos_id, width):
    """The definition: one forward per candidate over [prompt_b ; choice_c], log_softmax in float64 (token_logprobs).  Returns
    the terms float64 [B, C, width]: choice c's tokens in order, then its eos term when ``eos_id`` is not None; 0 behind them."""
    B, C = len(tries), max(len(t.sequences) for t in tries)
    terms = torch.zeros(B, C, width, dtype=torch.float64)
    for b, trie in enumerate(tries):
        prompt = embeddings[b:b + 1, : int(lens[b])]
        for c, q in enumerate(trie.sequences):
            o = model.lm(inputs_embeds=prompt, use_cache=True, past_key_values=None)
            logits = [o.logits[:, -1].float()]
            fed = list(q) if eos_id is not None else list(q[:-1])
            if fed:
                o = model.lm(input_ids=torch.tensor([fed], dtype=torch.int64, device=prompt.device), use_cache=True,
                             past_key_values=o.past_key_values)
                logits.append(o.logits[0, -len(fed):].float())
            want = list(q) + ([eos_id] if eos_id is not None else [])
            lp, _, _ = token_logprobs(torch.cat(logits, 0), torch.tensor(want, dtype=torch.int64))
            terms[b, c, : len(want)] = lp
    return terms


def _rank_engine(model, embeddings, lens, tries, eos_id, width, max_nodes):
    """rank() on the HIP engine: one prefill of the B prompts (its logits are the root's edges), then per group of choices one
    LMEngine.tree_forward over the trie's nodes against the same prompt cache, the fp32 head in slabs on the nodes that predict
    something (a node with children, a terminal node when eos counts), mg_token_logprobs_rows_f32 per edge.  The sums along the
    paths are per-level index ops on the device -- a gather of every candidate's terms, root first and the eos term last, and
    ``width`` adds in that fixed order: C x width floats, not a cost that a kernel of its own would move.  Returns (terms fp32
    [B, C, width], sums fp32 [B, C]) on the host."""
    from . import ops
    eng = model.lm.engine
    dev = eng.device
    B, C = len(tries), max(len(t.sequences) for t in tries)
    n_pos = eng.cfg.max_position_embeddings
    budget = n_pos - int(lens.max())
    if max_nodes is not None:
        budget = min(budget, int(max_nodes))
    made = {}
    for t in tries:
        if id(t) not in made:
            groups = rank_groups(t, budget)
            made[id(t)] = [t.rows(g) for g in groups], groups
    T_max = max(r.token.numel() for rs, _ in made.values() for r in rs)
    logits0, cache, _ = eng.prefill(embeddings.to(dev), cache_hint=T_max, reuse_cache=True, lengths=lens)
    terms, sums = torch.zeros(B, C, width), torch.full((B, C), float("-inf"))
    for g in range(max(len(rs) for rs, _ in made.values())):
        rows = [made[id(t)][0][g] if g < len(made[id(t)][0]) else None for t in tries]
        token, off, sub = pad_trie_rows(rows)
        T = token.shape[1]
        x = eng.tree_forward(cache, (token, off, sub))
        root_row, root_tok, need, tree_ent = [], [], [], []      # entries under the prompt's logits / under a node's logits
        per_row = []
        for b, r in enumerate(rows):
            if r is None:
                per_row.append(None)
                continue
            parent, term, tok = r.parent.tolist(), r.terminal.tolist(), r.token.tolist()
            feeds = set(parent) | ({i for i, v in enumerate(term) if v} if eos_id is not None else set())
            feeds.discard(-1)
            slot = {i: len(need) + k for k, i in enumerate(sorted(feeds))}       # node -> its row among the head's rows
            need += [b * T + i for i in sorted(feeds)]
            ent = {}                                                             # node -> ("r" | "t", index in that list)
            for i, pa in enumerate(parent):
                if pa < 0:
                    ent[i] = ("r", len(root_row))
                    root_row.append(b)
                    root_tok.append(tok[i])
                else:
                    ent[i] = ("t", len(tree_ent))
                    tree_ent.append((slot[pa], tok[i]))
            eos_ent = {}
            if eos_id is not None:
                for i, v in enumerate(term):
                    if v:
                        eos_ent[i] = ("t", len(tree_ent))
                        tree_ent.append((slot[i], eos_id))
            per_row.append((parent, ent, eos_ent, r.leaf_of.tolist()))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
        lp_root = torch.empty(len(root_row), dtype=torch.float32, device=dev)
        ops.token_logprobs_rows(logits0, i32(root_row).to(dev), i32(root_tok).to(dev), lp_root)
        order = sorted(range(len(tree_ent)), key=lambda e: tree_ent[e][0])
        where = [0] * len(order)
        for k, e in enumerate(order):
            where[e] = k
        lp_tree = eng.head_token_logprobs(x, torch.tensor(need, dtype=torch.int64), i32([tree_ent[e][0] for e in order]),
                                          i32([tree_ent[e][1] for e in order]))
        n_root, pad = len(root_row), len(root_row) + len(tree_ent)
        at = lambda e: e[1] if e[0] == "r" else n_root + where[e[1]]  # noqa: E731
        gather, dest = [], []
        for b, pr in enumerate(per_row):
            if pr is None:
                continue
            parent, ent, eos_ent, leaf_of = pr
            for c, leaf in zip(made[id(tries[b])][1][g], leaf_of):
                path, i = [], leaf
                while i >= 0:
                    path.append(at(ent[i]))
                    i = parent[i]
                path.reverse()                                                   # root first
                if eos_id is not None:
                    path.append(at(eos_ent[leaf]))
                gather.append(path + [pad] * (width - len(path)))
                dest.append(b * C + c)
        lp_ext = torch.cat([lp_root, lp_tree, torch.zeros(1, dtype=torch.float32, device=dev)])
        tv = lp_ext[torch.tensor(gather, dtype=torch.int64).to(dev)]            # [n, width]; + 0.0 behind a path changes nothing
        acc = tv[:, 0].clone()
        for d in range(1, width):
            acc = acc + tv[:, d]
        dest = torch.tensor(dest, dtype=torch.int64)
        terms.view(B * C, width)[dest] = tv.cpu()
        sums.view(B * C)[dest] = acc.cpu()
    return terms, sums


@torch.no_grad()
def rank(model, embeddings, choices, lengths=None, *, eos=True, length_penalty=0.0, max_nodes: int = None,
         return_terms: bool = False):
    """Rank a closed set of answers by their probability as whole sequences (Magma.rank; DESIGN.md "Ranking choices").
    ``embeddings`` / ``lengths``: what ``generate`` takes as a prompt (a (B, S, d) tensor, a list of per-row tensors, embed_batch's
    pair).  ``choices``: what ``choose`` takes -- a ``TokenTrie``, a list of token-id sequences or strings, or one of either per
    row.  Returns a ``Ranking``: ``logprobs[b, c]`` = sum_j log p(choice_c[j] | prompt_b, choice_c[:j]), plus
    log p(eos | prompt_b, choice_c) when ``eos`` (the model's eos id), all under the raw distribution -- the numbers
    ``Magma.score`` gives; ``count`` = the number of terms; ``scores = logprobs / count ** length_penalty``; ``index`` = the arg-max
    of ``scores``, the lowest position on an exact tie.  Columns follow the caller's list (a duplicate gets its score twice); rows
    with fewer than C choices are padded with -inf / 0.  ``return_terms=True`` returns (Ranking, terms fp32 [B, C, L + 1]): every
    term of the sums in order, 0 behind them.
    This function over an LM object without the engine is the definition: one forward per candidate over [prompt ; choice].  The
    HIP engine computes all choices of a row exactly in ONE forward over prompt + trie nodes: the prompt is prefilled once, the
    trie's nodes go through the blocks as one chunk in which every node attends to the prompt and to its own ancestors and sits
    at the position of its depth (LMEngine.tree_forward), so shared prefixes are computed once.  A trie with more nodes than free
    positions (``max_position_embeddings`` - prompt, or ``max_nodes``) is split into groups of whole choices, each its own tree
    against the same prompt cache.  ValueError: arguments ``choose`` refuses, ``eos`` that is no bool, a ``length_penalty`` that
    is not finite, a choice that would pass ``max_position_embeddings``."""
    if not isinstance(eos, bool):
        raise ValueError(f"eos must be True or False (the model's eos id counts or not), got {eos!r}")
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not math.isfinite(length_penalty):
        raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}")
    if max_nodes is not None and (isinstance(max_nodes, bool) or not isinstance(max_nodes, int) or max_nodes < 1):
        raise ValueError(f"max_nodes must be a positive integer, got {max_nodes!r}")
    embeddings, lengths = prompt_batch(embeddings, lengths, check=False)        # (rank's own wording for the lengths below)
    if not torch.is_tensor(embeddings) or embeddings.ndim != 3:
        raise ValueError("embeddings must be a (B, S, d) tensor, a list of per-row tensors or embed_batch's pair")
    B, S, _ = embeddings.shape
    tries = check_constraint_args(choices, B, getattr(getattr(model, "tokenizer", None), "encode", None), _logit_count(model))
    if tries is None:
        raise ValueError("rank() needs choices")
    if lengths is None:
        lens = torch.full((B,), S, dtype=torch.int64)
    else:
        lens = torch.as_tensor(lengths).detach().to("cpu")
        if lens.is_floating_point() or lens.dtype == torch.bool or lens.ndim != 1 or lens.shape[0] != B:
            raise ValueError(f"lengths must be {B} integers (one prompt length per row), got {lens.dtype} {tuple(lens.shape)}")
        lens = lens.to(torch.int64)
        if int(lens.min()) < 1 or int(lens.max()) > S:
            raise ValueError(f"every length must lie in [1, {S}], got {lens.tolist()}")
    n_pos = getattr(getattr(model.lm, "config", None), "max_position_embeddings", None)
    for b, t in enumerate(tries):
        if n_pos is not None and int(lens[b]) + t.max_len() > n_pos:
            raise ValueError(f"row {b}: the prompt ({int(lens[b])} positions) plus its longest choice ({t.max_len()} tokens) "
                             f"passes max_position_embeddings = {n_pos}")
    eos_id = int(model.eos_token) if eos else None
    C, width = max(len(t.sequences) for t in tries), max(t.max_len() for t in tries) + 1
    if getattr(model.lm, "device_token_selection", False):
        terms, sums = _rank_engine(model, embeddings, lens, tries, eos_id, width, max_nodes)
    else:
        t64 = _rank_host(model, embeddings, lens, tries, eos_id, width)
        terms, sums = t64.float(), t64.sum(-1).float()
    count = torch.zeros(B, C, dtype=torch.int64)
    for b, t in enumerate(tries):
        count[b, : len(t.sequences)] = torch.tensor([len(q) + int(eos) for q in t.sequences], dtype=torch.int64)
    live = count > 0
    logprobs = torch.where(live, sums, torch.full_like(sums, float("-inf")))
    scores = torch.where(live, logprobs / count.clamp(min=1).to(torch.float32) ** float(length_penalty), logprobs)
    best = scores.max(dim=1, keepdim=True).values
    index = torch.where(scores == best, torch.arange(C)[None, :], torch.full((1, 1), C)).min(dim=1).values
    out = Ranking(index.to(torch.int64), scores, logprobs, count)
    return (out, terms) if return_terms else out


class Explanation(NamedTuple):
    """What explain() returns: CPU tensors over the B rows and the U = most units of a row; columns past count[b] hold 0.0."""
    relevance: torch.Tensor        # fp32 [B, U]: perturbed_loss - loss[:, None]
    loss: torch.Tensor             # fp32 [B]: mean negative log-probability of the row's targets, unperturbed
    perturbed_loss: torch.Tensor   # fp32 [B, U]: the same with unit u suppressed
    count: torch.Tensor            # int64 [B]: the row's number of units

    def grid(self, b: int, start: int, height: int, width: int) -> torch.Tensor:
        """The relevance of the height * width units from ``start`` on as a (height, width) view -- the image-patch map when the
        default units are used and the image's tokens start at prompt position ``start`` (image_prefix lays them out row-major:
        12 x 12 for RN50x16 at 384 x 384)."""
        n = int(height) * int(width)
        if height < 1 or width < 1 or start < 0 or start + n > self.relevance.shape[1]:
            raise ValueError(f"grid of {height} x {width} units from {start} does not fit {self.relevance.shape[1]} units")
        return self.relevance[b, start: start + n].view(int(height), int(width))


def check_explain_args(suppression=0.9, similarity_threshold=None, batch_size=16):
    """The scalar arguments of explain(): 0 <= suppression <= 1 (the scale 1 - suppression c stays >= 0), a finite threshold or
    None, batch_size >= 1."""
    if isinstance(suppression, bool) or not isinstance(suppression, (int, float)) or not 0.0 <= float(suppression) <= 1.0:
        raise ValueError(f"suppression must be a number in [0, 1], got {suppression!r}")
    if similarity_threshold is not None and (isinstance(similarity_threshold, bool) or not isinstance(similarity_threshold, (int, float))
                                             or not math.isfinite(similarity_threshold)):
        raise ValueError(f"similarity_threshold must be a finite number or None, got {similarity_threshold!r}")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")


def explain_units(lens, units=None) -> List[List[List[int]]]:
    """The units of every row as lists of prompt positions.  None: one unit per prompt position.  Otherwise per row a list of
    non-empty position lists; a position outside [0, len_b) -- a target or a padding position -- raises."""
    lens = [int(v) for v in lens]
    if units is None:
        return [[[p] for p in range(n)] for n in lens]
    if len(units) != len(lens):
        raise ValueError(f"{len(units)} unit lists for {len(lens)} rows")
    out = []
    for b, (row, n) in enumerate(zip(units, lens)):
        chk = []
        for u in row:
            u = [int(p) for p in (u.tolist() if torch.is_tensor(u) else u)]
            if not u:
                raise ValueError(f"row {b}: an empty unit")
            if any(p < 0 or p >= n for p in u):
                raise ValueError(f"row {b}: unit {u} names a position outside the prompt [0, {n})")
            chk.append(u)
        out.append(chk)
    return out


def unit_scale(prompt, unit, suppression: float, similarity_threshold: float = None) -> torch.Tensor:
    """The scale vector of one unit over the n prompt positions of its row, fp32 [n] on the host.  Without a threshold: 1 - suppression
    on the unit's positions, 1.0 elsewhere.  With kappa: position k with c = max_{i in unit} cos(e_i, e_k) >= kappa gets
    1 - suppression c (the unit's own positions: c = 1); ``prompt`` (n, d) are the row's prompt embeddings, the cosine is taken in
    fp32 on the host so that the comparison with kappa is the same everywhere."""
    n = prompt.shape[0]
    idx = torch.tensor(unit, dtype=torch.int64)
    c = torch.zeros(n, dtype=torch.float32)
    if similarity_threshold is not None:
        e = prompt.detach().to("cpu", torch.float32)
        e = e / e.norm(dim=1, keepdim=True).clamp_min(1e-30)
        c = (e[idx] @ e.t()).max(dim=0).values.clamp(max=1.0)
        c = torch.where(c >= float(similarity_threshold), c, torch.zeros_like(c))
    c[idx] = 1.0
    return 1.0 - float(suppression) * c


def explain_work_list(n_units, batch_size: int) -> List[Tuple[int, int]]:
    """The rows explain() scores, as (b, u): per row its unperturbed copy (u = -1) and then its units, filled up with unperturbed
    copies of row 0 to a multiple of batch_size."""
    work = [(b, u) for b, n in enumerate(n_units) for u in range(-1, n)]
    return work + [(0, -1)] * (-len(work) % batch_size)


def mean_nll(logprobs: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """-sum_j logprobs[i, j] / count[i] in fp32 (positions past count[i] hold 0.0)."""
    return -(logprobs.to(torch.float32).sum(dim=1) / count.to(torch.float32))


def _explanation(work, losses, terms, n_units, return_terms):
    B, U = len(n_units), max(n_units)
    loss = torch.zeros(B, dtype=torch.float32)
    pert = torch.zeros(B, U, dtype=torch.float32)
    tm = torch.zeros(B, 1 + U, terms.shape[1], dtype=torch.float32)
    seen = set()
    for i, (b, u) in enumerate(work):
        if (b, u) in seen:          # the fill-up copies
            continue
        seen.add((b, u))
        tm[b, 1 + u] = terms[i]
        if u < 0:
            loss[b] = losses[i]
        else:
            pert[b, u] = losses[i]
    live = torch.arange(U)[None, :] < torch.tensor(n_units)[:, None]
    rel = torch.where(live, pert - loss[:, None], torch.zeros_like(pert))
    out = Explanation(rel, loss, pert, torch.tensor(n_units, dtype=torch.int64))
    return (out, tm) if return_terms else out


def explain_reference(model, embeddings, targets, lengths=None, *, suppression=0.9, units=None, similarity_threshold=None,
                      batch_size=16, return_terms=False):
    """The host statement of Magma.explain (DESIGN.md "Explaining an answer"), the plain loop: for every (row, unit) of the work
    list build the scale vector, score the row's targets with Magma.score(..., key_scale=) -- batch_size rows per call, every
    call padded to the same width -- and subtract the row's unperturbed loss."""
    check_explain_args(suppression, similarity_threshold, batch_size)
    embeddings, lens = prompt_batch(embeddings, lengths)
    B = embeddings.shape[0]
    lens = torch.full((B,), embeddings.shape[1], dtype=torch.int64) if lens is None else lens
    rows = [[int(v) for v in (r.tolist() if torch.is_tensor(r) else r) if int(v) != -100] for r in targets]
    W = max(int(n) + len(r) - 1 for n, r in zip(lens, rows))
    T = max(len(r) for r in rows)
    unit_rows = explain_units(lens, units)
    work = explain_work_list([len(u) for u in unit_rows], batch_size)
    losses, terms = [], []
    for i0 in range(0, len(work), batch_size):
        chunk = work[i0: i0 + batch_size]
        prompts, tgts, scales = [], [], []
        for b, u in chunk:
            n = int(lens[b])
            prompts.append(embeddings[b, :n])
            tgts.append(rows[b])
            ks = torch.ones(W, dtype=torch.float32)
            if u >= 0:
                ks[:n] = unit_scale(embeddings[b, :n], unit_rows[b][u], suppression, similarity_threshold)
            scales.append(ks)
        lp = model.score(prompts, tgts, key_scale=torch.stack(scales), width=W)
        terms.append(F.pad(lp.logprobs, (0, T - lp.logprobs.shape[1])))       # the chunk's widest row may be narrower than T
        losses.append(mean_nll(terms[-1], lp.count))
    return _explanation(work, torch.cat(losses), torch.cat(terms), [len(u) for u in unit_rows], return_terms)


def explain(model, embeddings, targets, lengths=None, *, suppression=0.9, units=None, similarity_threshold=None, batch_size=16,
            return_terms=False):
    """Magma.explain: the work list of explain_reference through LMEngine.score in forwards of one shape (batch_size, W).  The
    inputs are prepared once for the B rows ([prompt_b ; wte(targets_b[:-1])], the target positions) and gathered per forward on
    the device; the scale matrix of a forward is built on the host and copied once."""
    check_explain_args(suppression, similarity_threshold, batch_size)
    torch.cuda.set_device(model.device)
    eng = model.lm.engine
    if getattr(eng, "fp8_mode", False) and getattr(eng, "fp8_attn", False):
        raise NotImplementedError("key_scale is not implemented for the fp8 attention mode")
    prompts, _ = prompt_batch(embeddings, lengths)
    emb, tgt, tokens, count, lens, _ = model._score_inputs(embeddings, targets, lengths)
    B, W = tgt.shape
    T = tokens.shape[1]
    unit_rows = explain_units(lens, units)
    n_units = [len(u) for u in unit_rows]
    if max(n_units) < 1:
        raise ValueError("no row has a unit")
    host = [prompts[b, : int(lens[b])].detach().to("cpu", torch.float32) for b in range(B)] if similarity_threshold is not None \
        else [prompts[b, : int(lens[b])] for b in range(B)]      # one D2H copy per row, only the cosine needs it
    work = explain_work_list(n_units, batch_size)
    at = torch.arange(T)[None, :] < count[:, None]
    losses, terms = [], []
    for i0 in range(0, len(work), batch_size):
        chunk = work[i0: i0 + batch_size]
        idx = torch.tensor([b for b, _ in chunk], dtype=torch.int64)
        ks = torch.ones(len(chunk), W, dtype=torch.float32)
        for i, (b, u) in enumerate(chunk):
            if u >= 0:
                ks[i, : int(lens[b])] = unit_scale(host[b], unit_rows[b][u], suppression, similarity_threshold)
        lp, _, _ = eng.score(emb.index_select(0, idx.to(emb.device)), tgt[idx], 0, key_scale=ks)
        out = torch.zeros(len(chunk), T)
        out[at[idx]] = lp.cpu()
        losses.append(mean_nll(out, count[idx]))
        terms.append(out)
    return _explanation(work, torch.cat(losses), torch.cat(terms), n_units, return_terms)


def keep_conversation(cache, start: torch.Tensor, n_gen: int, eos_token, finish: Finish = None):
    """After a generate() call of n_gen kept steps whose first token sits at position start[b] of row b: every row keeps its
    generated tokens before its first eos.  A row that emitted eos is cut back to just before it (its later slots are
    overwritten by what comes next); a row that did not keeps its last token pending, to be fed first by the next call.
    ``finish`` (a per-row call's Finish): a row finished by an eos id at step f is cut back to just before it; a row finished by
    a stop sequence at step f keeps tokens 0 .. f, token f pending (the stop text is part of the conversation); the pad tokens
    fed after either wrote K / V past the row's position, which set_rows cuts off like the tokens after an eos."""
    hist = cache.history[:, :n_gen].cpu()                  # one host sync
    pos, pend = start.clone().to(torch.int64), torch.full((cache.B,), -1, dtype=torch.int64)
    if finish is not None:
        for r in range(cache.B):
            last = int(finish.kept[r]) - 1                 # the finishing step, or n_gen - 1 for an unfinished row
            pos[r] += last
            if finish.reason[r] != "eos":
                pend[r] = int(hist[r, last])
        cache.set_rows(pos, pend)
        return
    for r in range(cache.B):
        hits = (hist[r] == eos_token).nonzero() if eos_token is not None else torch.empty(0)
        if hits.numel():
            pos[r] += int(hits[0])
        else:
            pos[r] += n_gen - 1
            pend[r] = int(hist[r, n_gen - 1])
    cache.set_rows(pos, pend)


@torch.no_grad()
def _generate_beam(model, embeddings, max_steps, eos_token, decode, eos_check_every, lengths, k, length_penalty,
                   early_stopping, n_ret, return_scores, proc=None, groups=1, diversity=0.0):
    """generate()'s beam search over the prompt batch it has normalised: on the HIP engine's device, or beam_search on the host."""
    on_device = getattr(model.lm, "device_token_selection", False)
    embeddings, lengths = prompt_batch(embeddings, lengths, per_row=on_device)
    b, s, _ = embeddings.shape
    dev = embeddings.device
    with eval_mode(model):
        if on_device:
            beam = (k, length_penalty, early_stopping, int(max_steps)) + ((groups, diversity) if groups > 1 else ())
            run = _device_loop(model, embeddings, lengths, max_steps, eos_token, seed=None, every=poll_every(eos_check_every),
                               stop_on_eos=True, modes=dict(beam=beam, proc=proc), want_finish=False, past_key_values=None,
                               k=k, n_ret=n_ret)
            out, scores = run.out, run.scores
        else:
            emb = embeddings.repeat_interleave(k, dim=0)           # B prompts -> B*k rows, sample-major
            cache = {}

            def step(rows, tokens):
                if rows is None:
                    o = model.lm(inputs_embeds=emb, use_cache=True, past_key_values=None)
                else:
                    o = model.lm(input_ids=tokens[:, None].to(dev), use_cache=True,
                                 past_key_values=reorder_past(cache["past"], rows.to(dev)))
                cache["past"] = o.past_key_values
                return o.logits[:, -1, :].float()

            if groups > 1:
                toks, scores, _ = group_beam_search(step, b, k, groups, diversity, max_steps, eos_token, length_penalty,
                                                    early_stopping, n_ret, processors=proc)
            else:
                toks, scores, _ = beam_search(step, b, k, max_steps, eos_token, length_penalty, early_stopping, n_ret,
                                              processors=proc)
            out = layout_ids(toks.to(dev), s, lengths, model.image_token, eos_token, n_ret)
        if decode:
            out = decode_ids(model, out, eos_token)
    return (out, scores.float().cpu()) if return_scores else out


@torch.no_grad()
def _generate_contrastive(model, embeddings, max_steps, eos_token, decode, eos_check_every, lengths, k, alpha, stop_on_eos):
    """generate()'s contrastive search over the prompt batch it has normalised: on the HIP engine's device -- a cache of B * k rows,
    one token step per generated token behind the prefill, the first included --, or contrastive_search on the host."""
    on_device = getattr(model.lm, "device_token_selection", False)
    embeddings, lengths = prompt_batch(embeddings, lengths, per_row=on_device)
    b, s, _ = embeddings.shape
    dev = embeddings.device
    with eval_mode(model):
        if on_device:
            out = _device_loop(model, embeddings, lengths, max_steps, eos_token, seed=None, every=poll_every(eos_check_every),
                               stop_on_eos=stop_on_eos, modes=dict(contrast=(k, alpha)), want_finish=False,
                               past_key_values=None, k=k, first=False).out
        else:
            emb = embeddings.repeat_interleave(k, dim=0)           # B prompts -> B*k rows, sample-major
            cache = {}
            ln_f = getattr(getattr(model.lm, "transformer", None), "ln_f", None)

            def hidden(o):      # hidden_states[-1] of transformers' GPT-J: the output of ln_f
                h = o.hidden_states[-1]
                return ln_f(h) if ln_f is not None else h

            def step(tokens, parents):
                past = cache["past"] if parents is None else reorder_past(cache["past"], parents.to(dev))
                o = model.lm(input_ids=tokens[:, None].to(dev), use_cache=True, past_key_values=past, output_hidden_states=True)
                cache["past"] = o.past_key_values
                return o.logits[:, -1, :].float(), hidden(o)[:, -1, :]

            o = model.lm(inputs_embeds=emb, use_cache=True, past_key_values=None, output_hidden_states=True)
            cache["past"] = o.past_key_values
            toks, _ = contrastive_search(step, hidden(o)[::k], o.logits[::k, -1, :].float(), None, k, alpha, max_steps, eos_token,
                                         stop_on_eos)
            out = layout_ids(toks.to(dev), s, lengths, model.image_token, eos_token)
        if decode:
            out = decode_ids(model, out, eos_token)
    return out
