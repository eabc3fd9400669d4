"""Derived copies of the weights across writes to the weights: generate() after training steps reads the weights as they are now.

The engines keep many copies of the parameters -- the adapters' PackedLinear operands, [W_out | W_up], the folded down-projection,
[W_up_mlp | W_up_attn], the parallel adapters' scale vectors, the e4m3 / W8A16 / W4A16 operand sets, the training engine's _out_up /
_fp8_packs / _lm_train_packs, the encoder's re-laid-out convolutions and BatchNorm folds -- and the captured token steps hold raw
device addresses of all of them.  The parameters are written by code that goes round torch (AdamW through raw pointers, checkpoint
loading, _flush_bn_stats, resize_token_embeddings).  Every test here writes, then requires of the WARM engine -- operands, pooled
cache and captured steps made before the write -- the bits of a COLD model built from the live state dict (lifecycle_cases).  Two
conditions keep that from passing vacuously: the cold logits before and after the write differ at every compared step, and a
captured step existed on the very cache the second call received.

What the file was written against: LMEngine.repack_adapters replaced every adapter operand and left the graphs captured against
the old ones on the pooled caches and on caches the caller held, and generate() after step() without eval() read the packs from
before the step.  With those two repairs switched off and the replaced operands kept alive (stale values at valid addresses)
every test of items 1, 2 and 5 and the batch-statistics test fail at the first replayed step after the first write; the other
writers of item 3 (they replace the engine) and item 4 pass without them."""
import pytest
import torch

import kernel_compare as kc
import lifecycle_cases as L

pytestmark = pytest.mark.gpu


def step(cfg, loader, engine):
    from magma_amd.train_loop import train_step
    before = [g.master.clone() for g in engine.groups]
    engine.train()
    float(train_step(cfg, loader, engine))
    assert all(not torch.equal(a, g.master) for a, g in zip(before, engine.groups)), "the step moved nothing"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. optimizer steps with a frozen LM: the pooled cache and its graphs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(L.CASES))
def test_generate_after_optimizer_steps_equals_a_cold_model(dev, monkeypatch, case):
    """eval, generate, train, one real train_step, eval, generate on the same shapes -- twice in a row, as train.py does at every
    eval_every.  The LMEngine survives the steps (frozen LM), the second and third drive get the first one's pooled cache with its
    captured steps, and both must give the cold model's embeddings, logits (prefill and four token steps) and generate() tokens.
    One case per block shape that owns a derived adapter operand; the cold result of the last cycle is anchored to the fp32 oracle."""
    live = L.build(dev, monkeypatch, case)
    engine, loader, cfg = L.trainer(live)
    images, ids = L.inputs()
    engine.eval()
    lm_engine = live.lm.engine
    first = L.drive(live, images, ids)
    cold = L.drive(L.cold_of(dev, live, case), images, ids)
    L.assert_same(first, cold, f"{case}, before any step")
    st = first.cache.decode_state
    assert st.kinds == [L.KINDS[case]] * 2 and st.refusal is None, st.kinds
    assert L.has_derived(live, case), L.CASES[case][3]
    for cycle in (1, 2):
        assert first.cache.decode_state.graphs and next(iter(lm_engine._cache_pool.values())) is first.cache
        step(cfg, loader, engine)
        engine.eval()
        warm = L.drive(live, images, ids)
        assert live.lm.engine is lm_engine and warm.cache is first.cache, "the second call did not get the pooled cache"
        cold_model = L.cold_of(dev, live, case)
        before, cold = cold, L.drive(cold_model, images, ids)
        L.assert_moved(before, cold, f"{case}, step {cycle}")
        L.assert_same(warm, cold, f"{case}, after step {cycle}")
        assert L.has_derived(live, case)
    if L.CASES[case][2] is not None:
        L.anchor(cold_model, case, cold, images, ids)


SELECTIONS = {"sampled": dict(temperature=0.7, top_k=20, seed=11), "beam": dict(num_beams=2, return_scores=True),
              "ragged": dict(temperature=0.0, lengths=[5, 3])}


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_other_graph_keys_and_the_ragged_pool_entry(dev, monkeypatch, selection):
    """The same cycle at the default block shape through the public generate() with a fixed-seed sampled call, a beam call and a
    ragged call: other StepKeys, the beam buffers, and the pool's ragged entry."""
    live = L.build(dev, monkeypatch)
    engine, loader, cfg = L.trainer(live)
    images, ids = L.inputs()
    kw = dict(max_steps=L.STEPS, decode=False, stop_on_eos=False, **SELECTIONS[selection])

    def run(model):
        with torch.no_grad():
            out = model.generate(model.embed([images, ids]), **kw)
            again = model.generate(model.embed([images, ids]), **kw)       # on the pooled cache, replaying what the first call captured
        out, again = (out, again) if isinstance(out, tuple) else ((out,), (again,))
        assert all(torch.equal(a, b) for a, b in zip(out, again))
        (cache,) = model.lm.engine._cache_pool.values()
        assert cache.decode_state.graphs and cache.ragged == (selection == "ragged")
        return [t.clone() for t in out], cache

    engine.eval()
    first, cache = run(live)
    cold, _ = run(L.cold_of(dev, live))
    assert all(torch.equal(a, b) for a, b in zip(first, cold))
    for cycle in (1, 2):
        step(cfg, loader, engine)
        engine.eval()
        warm, warm_cache = run(live)
        assert warm_cache is cache, "the call after the step did not get the pooled cache"
        before, (cold, _) = cold, run(L.cold_of(dev, live))
        assert not all(torch.equal(a, b) for a, b in zip(before, cold)), f"step {cycle} changed nothing that {selection} generate() returns"
        for a, b in zip(warm, cold):
            assert torch.equal(a, b), (selection, cycle, a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. a cache the caller holds
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_detached_cache_continues_on_the_current_operands(dev, monkeypatch):
    """Prefill and four token steps (graphs captured), detach_cache, train step, eval; then the cache is continued -- extend with
    three new rows and four token steps under graphs -- and so is a clone of it that has no decode state, with use_graph=False.
    The K / V rows from before the step are the caller's business and the same in both; the logits of the new rows and steps
    must be equal, and differ from what the operands from before the step give (measured on a clone, eagerly, before the step)."""
    live = L.build(dev, monkeypatch)
    engine, loader, cfg = L.trainer(live)
    eng = live.lm.engine
    engine.eval()
    held = L.drive(live, emb=L.lm_inputs(live)).cache
    eng.detach_cache(held)
    assert not eng._cache_pool and held.decode_state.graphs
    more = L.lm_inputs(live, S=3, seed=8)

    @torch.no_grad()
    def continue_(cache, use_graph):
        o = eng.forward(inputs_embeds=more, use_cache=True, past_key_values=cache, cache_hint=L.STEPS)
        logits = [o.logits[:, -1].float().clone()]
        for _ in range(L.STEPS):
            logits.append(eng.decode(logits[-1].argmax(-1, keepdim=True), cache, use_graph=use_graph)[0].float().clone())
        return logits

    stale = continue_(L.clone_cache(held), False)
    step(cfg, loader, engine)
    engine.eval()
    assert live.lm.engine is eng
    clone = L.clone_cache(held)
    graphs = continue_(held, True)
    eager = continue_(clone, False)
    assert held.decode_state.graphs and not clone.decode_state.graphs
    for i, (a, b, c) in enumerate(zip(graphs, eager, stale)):
        assert not torch.equal(b, c), f"the step left the logits of continued step {i} as they were"
        assert torch.equal(a, b), f"continued step {i}: the held cache's step differs from the eager step on the current operands"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the other writers
# ---------------------------------------------------------------------------------------------------------------------------
def test_engine_load_checkpoint(dev, monkeypatch, tmp_path):
    """MagmaEngine.load_checkpoint under a live LMEngine, pooled cache and captured steps: back to the saved weights."""
    live = L.build(dev, monkeypatch)
    engine, loader, cfg = L.trainer(live)
    images, ids = L.inputs()
    step(cfg, loader, engine)
    engine.eval()
    engine.save_checkpoint(str(tmp_path), tag="a")
    saved = {k: v.clone() for k, v in live.state_dict().items()}
    step(cfg, loader, engine)
    engine.eval()
    L.drive(live, images, ids)
    before = L.drive(L.cold_of(dev, live), images, ids)
    path, _ = engine.load_checkpoint(str(tmp_path), tag="a")
    assert path is not None
    engine.eval()
    for k, v in live.state_dict().items():
        assert torch.equal(v, saved[k]), k
    warm = L.drive(live, images, ids)
    cold = L.drive(L.cold_of(dev, live), images, ids)
    L.assert_moved(before, cold, "load_checkpoint")
    L.assert_same(warm, cold, "after MagmaEngine.load_checkpoint")


def _scaled(sd, factor):
    pick = lambda k: (".adapter." in k or k.startswith("image_prefix.")) and sd[k].is_floating_point() and "running_" not in k  # noqa: E731
    return {k: (v * factor if pick(k) else v.clone()) for k, v in sd.items()}


def test_load_checkpoint_state_on_a_model_that_has_generated(dev, monkeypatch):
    live = L.build(dev, monkeypatch)
    images, ids = L.inputs()
    L.drive(live, images, ids)
    before = L.drive(L.cold_of(dev, live), images, ids)
    missing, unexpected = live.load_checkpoint_state(_scaled(live.state_dict(), 1.25))
    assert not unexpected
    warm = L.drive(live, images, ids)
    cold = L.drive(L.cold_of(dev, live), images, ids)
    L.assert_moved(before, cold, "load_checkpoint_state")
    L.assert_same(warm, cold, "after Magma.load_checkpoint_state")


def test_in_place_write_then_invalidate_packed(dev, monkeypatch):
    """torch writes to adapter, image_prefix and encoder parameters, then Magma.invalidate_packed() as its contract asks."""
    live = L.build(dev, monkeypatch)
    images, ids = L.inputs()
    L.drive(live, images, ids)
    before = L.drive(L.cold_of(dev, live), images, ids)
    with torch.no_grad():
        n = 0
        for name, p in live.named_parameters():
            if ".adapter." in name or name.startswith("image_prefix."):
                p.mul_(1.25)
                n += 1
    assert n > 20 and any(k.startswith("image_prefix.enc.") for k, _ in live.named_parameters())
    live.invalidate_packed()
    warm = L.drive(live, images, ids)
    cold = L.drive(L.cold_of(dev, live), images, ids)
    L.assert_moved(before, cold, "in-place write")
    L.assert_same(warm, cold, "after an in-place write and invalidate_packed")


def test_resize_token_embeddings_after_generate(dev, monkeypatch):
    """1056 -> 1099 -> 1061 rows in the embedding and the head (neither a multiple of 8: the head's padded width changes too),
    each after a generate call.  The new rows are random, so the cold model (which sniffs the sizes from the state dict) gets them
    from the live one."""
    live = L.build(dev, monkeypatch)
    images, ids = L.inputs()
    before = L.drive(live, images, ids)
    for rows in (1099, 1061):
        live.resize_token_embeddings(rows)
        assert live.lm.engine.V == rows and live.state_dict()["word_embedding.weight"].shape[0] == rows
        warm = L.drive(live, images, ids)
        cold_model = L.cold_of(dev, live)
        assert cold_model.lm.engine.V == rows
        cold = L.drive(cold_model, images, ids)
        assert warm.logits[0].shape == (2, rows) and before.logits[0].shape != warm.logits[0].shape
        L.assert_same(warm, cold, f"after resize_token_embeddings({rows})")
        before = warm


def test_batch_statistics_reach_the_batchnorm_folds(dev, monkeypatch):
    """A step in train(bn_batch_stats=True), then eval(): _flush_bn_stats writes the running statistics and the encoder's folds
    must follow; then a trainable-encoder step on the frozen statistics, for the re-laid-out convolutions.  Magma.embed([images])
    is the image path alone."""
    live = L.build(dev, monkeypatch)
    engine, loader, cfg = L.trainer(live)
    images, ids = L.inputs()
    engine.eval()
    L.drive(live, images, ids)
    cold = L.drive(L.cold_of(dev, live), images, ids)
    for mode in (True, False):
        stats = {k: v.clone() for k, v in live.state_dict().items() if "running_" in k}
        engine.train(bn_batch_stats=mode)
        step(cfg, loader, engine)
        engine.eval()
        moved = [k for k, v in live.state_dict().items() if "running_" in k and not torch.equal(v, stats[k])]
        assert (len(moved) == len(stats) > 10) if mode else not moved, (mode, len(moved), len(stats))
        warm = L.drive(live, images, ids)
        cold_model = L.cold_of(dev, live)
        before, cold = cold, L.drive(cold_model, images, ids)
        L.assert_moved(before, cold, f"bn_batch_stats={mode}")
        L.assert_same(warm, cold, f"after a step with bn_batch_stats={mode}")
        with torch.no_grad():
            a, b = live.embed([images]), cold_model.embed([images])
        assert torch.equal(a, b) and not torch.equal(a, before.emb[:, : a.shape[1]])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the training engine's own copies
# ---------------------------------------------------------------------------------------------------------------------------
TRAIN_KINDS = {"cat": ({}, {}, "cat"),
               "fp8_mx": ({"MAGMA_TRAIN_FP8": "1", "MAGMA_TRAIN_FP8_MX": "1", "MAGMA_FP8_ADAPTERS": "1"}, dict(mlp_factor=2), "fp8"),
               "freeze_lm_false": ({}, dict(freeze_lm=False), "serial")}


@pytest.mark.parametrize("kind", list(TRAIN_KINDS))
def test_training_forward_after_a_step_equals_emptied_caches(dev, monkeypatch, kind):
    """After a step, the training forward and backward on a fixed batch against the same engine with its caches emptied by hand
    (_out_up, _fp8_packs, _lm_train_packs, the weights epoch, Magma.invalidate_packed).  The loss is required equal.  The
    gradients are not bit-stable on this path (the column sums behind the BatchNorm and bias gradients are fp32 atomics): over
    three sessions on an MI355X two runs of the EMPTIED form differed, in the worst tensor -- a BatchNorm weight or bias of the
    trunk every time, another one from run to run --, by 1.5e-7 .. 1.8e-7 (cat), 1.0e-7 .. 1.4e-7 (fp8_mx) and 1.2e-7 .. 2.0e-7
    (freeze_lm_false) of the tensor's largest element; the loss was the same number every time.  The test prints the figure of
    its own run.  So every flat gradient is held to the per-element bound
    tests/test_grad_accumulation_gpu.py applies to the same tensors (kernel_compare.assert_accumulation with one part: the
    emptied run, its noise measured against a second emptied run)."""
    env, kw, mlp_kind = TRAIN_KINDS[kind]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from magma_amd.adapters import bump_weights_epoch
    from magma_amd.train_engine import MagmaEngine
    live = L.build(dev, monkeypatch, image_embed_dropout_prob=0.0, **kw)
    live.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(live)
    eng.train()
    g = torch.Generator().manual_seed(4)
    images = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    caps = torch.full((2, live.seq_len), live.eos_token, dtype=torch.int64)
    caps[0, :23], caps[1, :11] = torch.randint(0, 1000, (23,), generator=g), torch.randint(0, 1000, (11,), generator=g)

    def run():
        for grp in eng.groups:
            grp.grad.zero_()
        eng.micro_steps = 0
        out = eng(images, caps.to(dev))
        eng.backward(out.loss)
        return float(out.loss), [grp.grad.clone() for grp in eng.groups]

    def emptied():
        eng._out_up, eng._fp8_packs, eng._lm_train_packs = {}, {}, None
        bump_weights_epoch()
        live.invalidate_packed()
        return run()

    loss0, g0 = run()
    assert eng._train_block_kind(0).mlp == mlp_kind
    eng.step()                                     # the real update, from the gradients of that run
    assert eng.global_steps == 1
    loss_w, warm = run()
    loss_c, cold = emptied()
    loss_r, repeat = emptied()
    assert loss_w != loss0 and not any(torch.equal(a, b) for a, b in zip(g0, cold)), "the step changed nothing"
    assert loss_w == loss_c == loss_r, (loss_w, loss_c, loss_r)
    view = lambda flats, p: eng.groups[eng._where[id(p)][0]].view(flats[eng._where[id(p)][0]], p)  # noqa: E731
    seen, fails, noise = set(), [], (0.0, "")
    for name, p in live.named_parameters():
        if not eng.is_trainable(p) or id(p) in seen:
            continue
        seen.add(id(p))
        c, r = view(cold, p), view(repeat, p)
        noise = max(noise, (float((c - r).abs().max() / (c.abs().max() + 1e-30)), name))
        try:
            res = kc.assert_accumulation(view(warm, p), [c], [r], f"{kind} {name}")
            assert not res["zero_parts"] or not name.endswith(("weight", "bias")), f"{name}: identically zero gradient"
        except AssertionError as e:
            fails.append(str(e))
    print(f"[lifecycle] {kind}: {len(seen)} tensors; two emptied runs differ by at most {noise[0]:.3g} of a tensor's max ({noise[1]})")
    assert len(seen) == sum(len(grp.params) for grp in eng.groups)
    assert not fails, f"{len(fails)} tensor(s):\n" + "\n".join(fails[:8])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. generate() without eval()
# ---------------------------------------------------------------------------------------------------------------------------
def test_generate_straight_after_a_step_uses_the_current_weights(dev, monkeypatch):
    """Decided behaviour: generate() after step() WITHOUT eval() computes with the weights as they are.  (LM inputs are given as
    embeddings: the module is in training mode, where Magma.embed drops image features at random.)  eval() afterwards changes
    nothing."""
    live = L.build(dev, monkeypatch)
    engine, loader, cfg = L.trainer(live)
    emb = L.lm_inputs(live)
    engine.eval()
    first = L.drive(live, emb=emb)
    before = L.drive(L.cold_of(dev, live), emb=emb)
    L.assert_same(first, before, "before the step")
    step(cfg, loader, engine)
    assert engine.training
    warm = L.drive(live, emb=emb)
    assert warm.cache is first.cache
    cold = L.drive(L.cold_of(dev, live), emb=emb)
    L.assert_moved(before, cold, "the step")
    L.assert_same(warm, cold, "generate() straight after step()")
    engine.eval()
    L.assert_same(L.drive(live, emb=emb), cold, "after the eval() that follows")
