"""Rows, parameter grid and comparisons shared by the tests of transformers' sampler (tests/test_nucleus_sampling_cpu.py,
tests/test_nucleus_sampling_gpu.py) and by the generator of their pins (tests/golden/make_warper_golden.py).

Row kinds: ``peaked`` (one token holds nearly all the mass), ``flat`` (every probability ~ 1 / V), ``randn``, ``randn3``
(randn * 3) -- these four made TIE-FREE: equal values are moved apart by single ulps, so that a kept SET is well defined -- and
``bf16`` (randn * 0.5 rounded to bf16: many exact ties, also at the boundaries of every rule)."""
import itertools

import torch

TIE_FREE = ("peaked", "flat", "randn", "randn3")
KINDS = TIE_FREE + ("bf16",)
_SEED = {"peaked": 1, "flat": 2, "randn": 3, "randn3": 4, "bf16": 5}
# (temperature, top_k, top_p, min_p)
GRID = tuple(itertools.product((0.7, 1.0, 1.3), (0, 40, 1000), (0.9, 0.3, 1.0), (0.0, 0.05)))


def untie(x):
    """Every row's equal values moved apart by single ulps (upwards, in sorted order) until all are distinct."""
    x = x.clone()
    for r in range(x.shape[0]):
        v, order = torch.sort(x[r])
        while True:
            dup = v[1:] <= v[:-1]
            if not bool(dup.any()):
                break
            nxt = torch.nextafter(v[:-1], torch.full_like(v[:-1], float("inf")))
            v[1:] = torch.where(dup, nxt, v[1:])
        x[r, order] = v
    return x


def make_rows(kind, B, V, seed_offset=0):
    g = torch.Generator().manual_seed(_SEED[kind] + 100 * seed_offset)
    x = torch.randn(B, V, generator=g)
    if kind == "peaked":
        x = x * 4.0
        x[:, 17 % V] = 30.0       # the rest sums to about V e^8 = e^18.8 at V = 50 258: this token holds 1 - e^-11 of the mass
    elif kind == "flat":
        x = x * 0.01
    elif kind == "randn3":
        x = x * 3.0
    elif kind == "bf16":
        return (x * 0.5).to(torch.bfloat16).float()
    return untie(x)


def transformers_kept(x, temperature, top_k, top_p, min_p):
    """Kept mask (R, V) of transformers' chained warpers, as GenerationMixin._get_logits_processor chains them for
    do_sample=True (a neutral value leaves its warper out), on float64 scores."""
    from transformers.generation.logits_process import (MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    s = x.double()
    ids = torch.zeros(x.shape[0], 1, dtype=torch.long)
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(ids, s)
    if top_k > 0:
        s = TopKLogitsWarper(top_k=int(top_k), min_tokens_to_keep=1)(ids, s)
    if 0.0 < top_p < 1.0:
        s = TopPLogitsWarper(top_p=float(top_p), min_tokens_to_keep=1)(ids, s)
    if min_p > 0.0:
        s = MinPLogitsWarper(min_p=float(min_p), min_tokens_to_keep=1)(ids, s)
    return ~torch.isneginf(s)


def host_kept(x, temperature, top_k, top_p, min_p):
    from magma_amd import sampling as S
    return ~torch.isneginf(S.warp_filter(x, temperature, top_k, top_p, min_p))


def count_diff(row, kept_a, kept_b):
    """Sum over the distinct values of ``row`` of |survivors in a - survivors in b|: 0 when the two kept sets differ only in
    WHICH of several equal values they hold."""
    d = kept_a != kept_b
    off = 0
    for v in row[d].unique():
        sel = row == v
        off += abs(int(kept_a[sel].sum()) - int(kept_b[sel].sum()))
    return off


def pack(mask):
    """bool (..., V) -> uint8 (..., ceil(V / 8))"""
    import numpy as np
    return torch.from_numpy(np.packbits(mask.numpy(), axis=-1))


def unpack(bits, V):
    import numpy as np
    return torch.from_numpy(np.unpackbits(bits.numpy(), axis=-1)[..., :V].astype(bool))
