"""Choosing over a request stream at full width (d 4096, 16 heads, ff 16384, V 50258, one block): five requests through a slot
session of two slots, every request against the fp32 CPU oracle's constrained greedy walk of that request ALONE -- the oracle's
logits masked to ``TokenTrie.allowed`` at every step -- by the rule and ORACLE_MARGIN of tests/test_stream_fullwidth_gpu.py: ids are
compared up to the first decision (between the two best ALLOWED tokens) within the margin, and where no decision of a request is
within it, its ``choice`` is asserted equal.

Prompts: the seeds of tests/test_stream_fullwidth_gpu.py.  Every request's choices hold the first three tokens of the oracle's own
free greedy decode, a sibling that leaves it after two, and unrelated sequences, so the walk is three decisions deep."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fullwidth_common as F  # noqa: E402
from test_continue_generate_gpu import ORACLE_MARGIN  # noqa: E402
from test_stream_fullwidth_gpu import LENS, SEEDS  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EOS = 50257


def oracle_choose(lm, cfg, emb, trie):
    """(ids with the final eos, per step the gap between the two best allowed logits in units of std(logits); inf when forced)."""
    from oracle.model import lm_forward
    ids, gaps, past = [], [], None
    for i in range(trie.max_len() + 1):
        with torch.no_grad():
            r = lm_forward(lm, cfg, inputs_embeds=emb, past=None) if i == 0 else \
                lm_forward(lm, cfg, input_ids=torch.tensor([[ids[-1]]]), past=past)
        logits, past = r["logits"][0, -1].float(), r["past_key_values"]
        allowed = sorted(trie.allowed(ids, [EOS]))
        vals = logits[torch.tensor(allowed)]
        order = torch.argsort(vals, descending=True, stable=True)
        gaps.append(float("inf") if len(allowed) == 1 else float(vals[order[0]] - vals[order[1]]) / float(logits.std()))
        ids.append(allowed[int(order[0])])
        if ids[-1] == EOS:
            break
    return ids, gaps


def test_five_requests_two_slots_equal_the_oracle_alone(dev):
    from magma_amd.sampling import TokenTrie, choose_stream
    from magma_amd.testing import build_reduced_magma
    from oracle.model import generate_greedy
    cfg = F.full_width_config(enc_width=16, enc_layers=(1, 1, 2, 1))
    params = F.full_width_params(cfg)
    model = build_reduced_magma(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=cfg.n_positions, enc_width=16,
                                enc_layers=(1, 1, 2, 1))
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing[:4], unexpected[:4])
    model.eval()
    lm = F.lm_only(params)
    prompts = [torch.randn(n, cfg.d_model, generator=torch.Generator().manual_seed(s)).to(BF16) for n, s in zip(LENS, SEEDS)]
    g = torch.Generator().manual_seed(5)
    sets = []
    for p, n in zip(prompts, LENS):
        with torch.no_grad():
            toks, _ = generate_greedy(lm, cfg, p.float()[None], 3, stop_on_eos=False)
        own = [t for t in toks[0, n:].tolist()]
        x = [t for t in torch.randint(0, 50000, (12,), generator=g).tolist() if t not in own][:6]
        sets.append([own[:2] + x[:1], own, x[1:3], x[3:4], own[:1], x[4:6]] if EOS not in own else [x[:2], x[2:3]])
    shared = TokenTrie(sets[4])
    sets[1] = sets[4] = shared
    got = list(choose_stream(model, [(p.to(dev), c) for p, c in zip(prompts, sets)], slots=2, every=3, max_choice_tokens=4, max_prompt=64,
                             eos_token=[EOS], top_logprobs=2))
    assert sorted(r.index for r in got) == list(range(5)) and {r.slot for r in got} == {0, 1}
    compared = total = decided = 0
    for r in sorted(got, key=lambda r: r.index):
        trie = sets[r.index] if isinstance(sets[r.index], TokenTrie) else TokenTrie(sets[r.index])
        ids = r.tokens.tolist()
        ref, gaps = oracle_choose(lm, cfg, prompts[r.index].float()[None], trie)
        assert ids[-1] == EOS and r.reason == "eos" and r.choice == trie.index(ids[:-1]) >= 0, r
        assert r.logprobs.shape == (len(ids),) and r.top_ids.shape == (len(ids), 2) and bool((r.logprobs <= 0).all())
        total += len(ids)
        clear = True
        for i, x in enumerate(ids):
            if i >= len(gaps) or gaps[i] <= ORACLE_MARGIN:
                clear = False
                break
            assert x == ref[i], f"request {r.index}, token {i}: engine {x} != oracle {ref[i]} (engine {ids}, oracle {ref})"
            compared += 1
        if clear:
            assert r.choice == trie.index(ref[:-1]), (r, ref)
            decided += 1
    print(f"compared {compared} of {total} tokens ({compared / total:.0%}); the oracle's margin decides {decided} of 5 choices")
    assert decided >= 3, (decided, compared, total)
