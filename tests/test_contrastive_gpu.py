"""Contrastive search on the device (DESIGN.md "Contrastive search"): generate(penalty_alpha=, top_k=) on the reduced model
against the host statement magma_amd.sampling.contrastive_search driven by the engine's own kernels -- eager decode steps over
the B * k rows and ops.layernorm for the hidden states, so both sides see the same bits --, with every selection asserted decided
under the derived bound (tests/contrastive_cases.py); then its properties, its launch sequence and one full-width case."""
import pytest
import torch

import contrastive_cases as CC
from launch_trace import OPS, SELECT_OPS, record

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
CONTRAST_OPS = ("contrastive_sim", "contrastive_finish", "kv_broadcast", "contrastive_topk")
ALL_OPS = tuple(dict.fromkeys(OPS + SELECT_OPS + CONTRAST_OPS))


def _model(dev, **kw):
    from magma_amd.testing import build_reduced_magma
    torch.manual_seed(0)
    model = build_reduced_magma(dev, **kw)
    model.eval()
    with torch.no_grad():
        # a trained head is peaked; the random one is nearly uniform (logits within +-1), which leaves the candidates' probabilities --
        # and with them all scores of a step -- within 1e-3 of each other, the scale of the error bound itself.  Six times the
        # weights give top probabilities of 0.05 to 0.5; the penalty still decides steps (asserted below)
        model.lm.lm_head.weight *= 6.0
        model.lm.lm_head.bias[model.eos_token] += 4.0       # eos within reach
        model.lm.invalidate_packed()
    return model


def _emb(model, B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, model.lm.config.hidden_size, generator=g).to(BF16).to(model.device)


def _host_on_engine(model, emb, k, alpha, n, lengths=None, stop_on_eos=True):
    """The host statement driven by the engine's own kernels: one prefill over the B * k rows, eager greedy-plan decode steps on
    that cache with the rows re-gathered by index, and the op the engine takes every hidden state from (ops.layernorm with ln_f's
    parameters on the bf16 block output) -- the same kernels on the same cache contents, so the same logits and hidden rows."""
    from magma_amd import ops
    from magma_amd.sampling import contrastive_search
    eng = model.lm.engine
    B, S, d = emb.shape
    emb_k = emb.repeat_interleave(k, dim=0)
    kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths).repeat_interleave(k)}
    o = eng.forward(inputs_embeds=emb_k, use_cache=True, cache_hint=n, output_hidden_states=True, **kw)
    c = o.past_key_values
    ln = lambda x: ops.layernorm(x, eng.lnf_g, eng.lnf_b, eng.eps)  # noqa: E731
    prompt_hidden = ln(o.hidden_states[-1][::k].reshape(B * S, d)).view(B, S, d)

    def step(tokens, parents):
        if parents is not None:
            r = parents.to(model.device)
            c.k.copy_(c.k.index_select(1, r))
            c.v.copy_(c.v.index_select(1, r))
        lg, _ = eng.decode(tokens.view(-1, 1).to(model.device), c, use_graph=False)
        st = c.decode_state
        x = st.xa if eng.L % 2 == 0 else st.xb          # the last block's output (the blocks alternate between the two)
        return lg.float().cpu(), ln(x).cpu()

    return contrastive_search(step, prompt_hidden.cpu(), o.logits[::k, -1].float().cpu(), lengths, k, alpha, n, model.eos_token,
                              stop_on_eos)


def _generated(out, S, n, lengths):
    if lengths is None:
        return out[:, S: S + n].cpu()
    return torch.stack([out[i, int(m): int(m) + n].cpu() for i, m in enumerate(lengths)])


def _check_against_host(model, emb, k, alpha, n, lengths=None, stop_on_eos=True):
    from magma_amd.sampling import contrastive_margin
    ref, rec = _host_on_engine(model, emb, k, alpha, n, lengths, stop_on_eos)
    d = emb.shape[2]
    margin, need = contrastive_margin(rec), CC.gap_bound(alpha, d)
    print(f"B {emb.shape[0]} k {k} d {d}: {len(rec)} steps, smallest gap {margin:.3e} (decided above {need:.3e})")
    assert margin > need, (margin, need)               # every step decided; an input drifting into a tie fails here
    out = model.generate(emb, max_steps=n, penalty_alpha=alpha, top_k=k, decode=False, lengths=lengths, stop_on_eos=stop_on_eos)
    assert out.shape == (emb.shape[0], emb.shape[1] + ref.shape[1])
    got = _generated(out, emb.shape[1], ref.shape[1], lengths)
    assert torch.equal(got, ref), (got, ref)
    return out, ref, rec


# ``seed``: the prompt embeddings.  24 selections among scores that lie within a few 1e-2 of each other come within 1e-4 of a tie
# for about one seed in four; each seed below is one at which the REFERENCE's smallest gap is more than 18 times the bound (measured
# over seeds 60 .. 71, by the host statement alone).  The decidedness assertion stays: a change that moves an input into a tie fails it.
CONFIGS = {
    "v1": dict(seed=66),
    "ragged": dict(seed=68, lengths=[7, 4, 5]),
    "wide": dict(seed=66, B=5),                          # 20 rows: the eager tile-GEMM step
    "k16": dict(seed=60, B=1, k=16),
    "v2": dict(seed=66, build=dict(mlp_factor=4, attn_factor=4)),
    "parallel": dict(seed=61, build=dict(adapter_config={"mlp": dict(adapter_type="parallel", downsample_factor=4),
                                                         "attention": dict(adapter_type="scaled_parallel", downsample_factor=8)})),
    "w4a16": dict(seed=61, env="MAGMA_DECODE_W4", build=dict(n_layer=2, n_head=4, d_ff=2048, mlp_factor=2)),
    "w8a16": dict(seed=65, env="MAGMA_DECODE_W8", build=dict(n_layer=2, n_head=4, d_ff=2048, mlp_factor=1)),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_engine_equals_host_statement(dev, monkeypatch, cfg):
    c = CONFIGS[cfg]
    if "env" in c:
        monkeypatch.setenv(c["env"], "1")
    model = _model(dev, **c.get("build", {}))
    if "env" in c:
        assert model.lm.engine._quantised_decode() is not None
    emb = _emb(model, c.get("B", 3), 7, seed=c["seed"])
    out, ref, rec = _check_against_host(model, emb, c.get("k", 4), 0.6, 8, lengths=c.get("lengths"), stop_on_eos=False)
    assert ref.shape[1] == 8
    picked = torch.stack([r["selected"] for r in rec])
    assert cfg == "k16" or bool((picked > 0).any())      # the penalty, not the probability alone, decided some step


def test_top_k_one_is_greedy(dev):
    model = _model(dev)
    emb = _emb(model, 3, 6, seed=2)
    a = model.generate(emb, max_steps=10, temperature=0.0, decode=False)
    b = model.generate(emb, max_steps=10, penalty_alpha=0.6, top_k=1, decode=False)
    assert torch.equal(a, b)
    lengths = [6, 3, 5]
    a = model.generate(emb, max_steps=10, temperature=0.0, decode=False, lengths=lengths)
    b = model.generate(emb, max_steps=10, penalty_alpha=1.0, top_k=1, decode=False, lengths=lengths)
    assert torch.equal(a, b)


def test_graph_equals_eager_sample_alone_and_nothing_leaks(dev, monkeypatch):
    model = _model(dev)
    emb = _emb(model, 3, 6, seed=9)
    kw = dict(max_steps=10, penalty_alpha=0.6, top_k=4, decode=False)
    a = model.generate(emb, **kw)
    b = model.generate(emb, **kw)                        # the second call replays the captured step
    assert torch.equal(a, b)
    eng = model.lm.engine
    assert any(key.contrast for c in eng._cache_pool.values() for key in c.decode_state.graphs)
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **k2: orig(*x, **{**k2, "use_graph": False}))
    c = model.generate(emb, **kw)
    monkeypatch.undo()
    assert torch.equal(a, c)
    for i in range(3):          # each sample alone equals its row of the batch, up to where either call stopped (the all-eos rule)
        o = model.generate(emb[i: i + 1], **kw)
        n = min(o.shape[1], a.shape[1])
        assert n > emb.shape[1] and torch.equal(o[0, :n], a[i, :n])
    # other values of k and alpha on the same cache: the buffers are re-armed, the steps captured for (4, 0.6) are not replayed
    fresh = _model(dev)
    for more in (dict(penalty_alpha=0.3, top_k=4), dict(penalty_alpha=0.6, top_k=2)):
        assert torch.equal(model.generate(emb, max_steps=10, decode=False, **more), fresh.generate(emb, max_steps=10, decode=False, **more))
    # greedy and sampled calls on the same model afterwards equal those of a fresh model: nothing leaked
    emb12 = _emb(model, 12, 6, seed=10)                  # the 12-row cache the contrastive calls used
    for e, call in ((emb12, dict(temperature=0.0)), (emb12, dict(temperature=0.8, seed=5)), (emb, dict(num_beams=4))):
        assert torch.equal(model.generate(e, max_steps=8, decode=False, **call), fresh.generate(e, max_steps=8, decode=False, **call))
    assert torch.equal(model.generate(emb, **kw), a)


def test_default_is_the_call_as_it_was(dev):
    """penalty_alpha = 0.0 equals the call without the keyword: ids and the recorded launch sequence, on fresh models (a pooled
    cache would replay its graph, which records nothing); nothing contrastive is allocated."""
    emb = None
    runs = []
    for kw in (dict(), dict(penalty_alpha=0.0), dict(penalty_alpha=0.0, top_k=5)):
        model = _model(dev)
        emb = _emb(model, 2, 6, seed=3) if emb is None else emb
        temp = dict(temperature=0.0) if "top_k" not in kw else dict(temperature=0.7, seed=11)
        recs, out = record(model.lm.engine, lambda: model.generate(emb, max_steps=6, decode=False, **temp, **kw), op_names=ALL_OPS)
        assert not isinstance(out, Exception), out
        assert all(c.contrast is None and c.prefill_x is None for c in model.lm.engine._cache_pool.values())
        assert not any(r["op"] in CONTRAST_OPS for r in recs)
        runs.append(([r["op"] for r in recs], out))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and "argmax" in runs[0][0]
    model = _model(dev)
    recs, out = record(model.lm.engine, lambda: model.generate(emb, max_steps=6, decode=False, temperature=0.7, seed=11, top_k=5),
                       op_names=ALL_OPS)
    assert [r["op"] for r in recs] == runs[2][0] and torch.equal(out, runs[2][1]) and "sample" in runs[2][0]


def test_launch_count_of_the_step(dev):
    """The contrastive step = the greedy step over the same R rows, minus the argmax and its bookkeeping, plus ln_f, the similarity,
    the selection, the K / V broadcast and the next top-k: three launches more."""
    from magma_amd.engine import LMEngine
    model = _model(dev)
    eng = model.lm.engine
    B, k = 2, 4
    emb = _emb(model, B, 6, seed=4).repeat_interleave(k, dim=0)
    greedy = LMEngine.selection_plan(vocab=eng.V)
    plan = LMEngine.selection_plan(contrast=(k, 0.6), vocab=eng.V)
    with torch.no_grad():
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=8, eos_token=model.eos_token, plan=greedy)
        g_recs, res = record(eng, lambda: eng.decode(None, o.past_key_values, use_graph=False, plan=greedy),
                             cache=o.past_key_values, op_names=ALL_OPS)
        assert not isinstance(res, Exception), res
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=8, eos_token=model.eos_token, plan=plan)
        c_recs, res = record(eng, lambda: eng.decode(None, o.past_key_values, use_graph=False, plan=plan),
                             cache=o.past_key_values, op_names=ALL_OPS)
        assert not isinstance(res, Exception), res
    g_ops, c_ops = [r["op"] for r in g_recs], [r["op"] for r in c_recs]
    assert g_ops[-2:] == ["argmax", "sample_finish"]
    assert c_ops == g_ops[:-2] + ["layernorm", "contrastive_sim", "contrastive_finish", "kv_broadcast", "contrastive_topk"]
    print(f"greedy step over {B * k} rows: {len(g_ops)} launches; contrastive step: {len(c_ops)}")
    assert len(c_ops) == len(g_ops) + 3


def test_cached_step_needs_an_armed_cache(dev):
    from magma_amd.engine import LMEngine
    model = _model(dev)
    eng = model.lm.engine
    emb = _emb(model, 4, 5, seed=5)
    with torch.no_grad():
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=4, eos_token=model.eos_token)
        with pytest.raises(ValueError, match="armed"):
            eng.decode(None, o.past_key_values, plan=LMEngine.selection_plan(contrast=(2, 0.6), vocab=eng.V))
        with pytest.raises(ValueError, match="samples x top_k"):
            eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=4, eos_token=model.eos_token,
                        plan=LMEngine.selection_plan(contrast=(3, 0.6), vocab=eng.V))


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block, B = 2, k = 4: the full-width top-k, similarity and selection inside the captured step."""
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    emb = _emb(model, 2, 5, seed=61)                     # (a seed chosen as those of CONFIGS)
    _check_against_host(model, emb, 4, 0.6, 6, stop_on_eos=False)
