"""What tests/test_weight_lifecycle_gpu.py shares: the block shapes that own a derived copy of an adapter weight, the reduced models,
the drive whose logits and tokens are compared, the COLD model of a live one, and the fp32-oracle anchor of the cold result.

The oracle of every test there: after a write to the weights the warm engine (packed operands, pooled caches and captured token
steps made BEFORE the write) computes what a cold one computes -- a second model from build_reduced_magma with the same arguments
and switches, loaded through load_checkpoint_state(live.state_dict()) -- bit for bit: the same kernels, launches and parameter bits."""
from typing import NamedTuple

import torch

BF16 = torch.bfloat16
STEPS = 4            # cache_hint / max_steps: one eager token step, one capture, two replays
LR = 2e-3            # AdamW's first update is lr * sign(g): a tenth of the amplified adapter weights (std 2e-2)

_LN = dict(adapter_type="normal", downsample_factor=4, add_layernorm=True)
# id -> (switches set before the model is built, build_reduced_magma arguments, OracleConfig.tiny arguments or None = not anchored,
#        the derived operand of engine.layers[0] that must exist once a token step has run, as a path of attributes)
CASES = {
    "fold2": ({}, {}, {}, ("out_up",)),
    "fold1": ({"MAGMA_DECODE_FOLD": "1"}, {}, {}, ("fc_dn",)),
    "fold0": ({"MAGMA_DECODE_FOLD": "0"}, {}, {}, ("mlp_adapter",)),
    "v2": ({}, dict(mlp_factor=8, attn_factor=8), dict(mlp_adapter_hidden=64, attn_adapter_hidden=64), ("up_cat",)),
    "scaled_parallel": ({}, dict(attn_factor=8, attn_type="scaled_parallel"),
                        dict(attn_adapter_hidden=64, attn_adapter_type="scaled_parallel"), ("attn_par",)),
    "layernorm": ({}, dict(adapter_config={"mlp": dict(_LN), "attention": dict(_LN, downsample_factor=8)}),
                  dict(attn_adapter_hidden=64, adapter_layernorm=True), ("attn_ad_ln",)),
    "w4": ({"MAGMA_DECODE_W4": "1"}, dict(n_head=4, mlp_factor=2), dict(n_head=4, mlp_adapter_hidden=512), ("w4", "mlp_adapter")),
    "w8": ({"MAGMA_DECODE_W8": "1"}, dict(n_head=4, mlp_factor=1), dict(n_head=4, mlp_adapter_hidden=1024), ("w8", "mlp_adapter")),
    # the prefill's e4m3 copies; the block shape is fold2's, anchored there (the fp8 prefill has its own bound, tests/test_fp8_gpu.py)
    "fp8_attn": ({"MAGMA_FP8": "attn"}, {}, None, ("fp8",)),
}
KINDS = {"fold2": "fold2", "fold1": "fold1", "fold0": "grouped", "v2": "v2", "scaled_parallel": "generic", "layernorm": "generic",
         "w4": "grouped", "w8": "grouped", "fp8_attn": "fold2"}


def build(dev, monkeypatch, case="fold2", **extra):
    """The reduced model of ``case`` (2 blocks, d = 512 or 1024, n_positions 128) with its switches set, the adapter projections
    20 x their 1e-3 init so that their arithmetic shows in the logits, and a learning rate that holds from the first step (the
    schedule's warm-up starts at min_lr)."""
    from magma_amd.testing import build_reduced_magma
    env, kw, _, _ = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(0)
    model = build_reduced_magma(dev, n_positions=128, lr=LR, min_lr=LR, image_enc_lr=LR, **kw, **extra)
    with torch.no_grad():
        for n, p in model.lm.named_parameters():
            if ".adapter." in n and p.ndim == 2:
                p.mul_(20.0)
    model.invalidate_packed()
    model.eval()
    return model


def cold_of(dev, live, case="fold2", **extra):
    """A model that has never computed anything, with ``live``'s parameters and buffers as they are now."""
    from magma_amd.testing import build_reduced_magma
    _, kw, _, _ = CASES[case]
    cold = build_reduced_magma(dev, n_positions=128, lr=LR, min_lr=LR, image_enc_lr=LR, **kw, **extra)
    missing, unexpected = cold.load_checkpoint_state(live.state_dict())
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") or k.startswith(("transformer.", "word_embedding.")) for k in missing), missing
    cold.eval()
    return cold


def trainer(model):
    """(MagmaEngine, endless loader of SyntheticImgCptDataset batches of 2, config) with windows of one micro-step."""
    from magma_amd.datasets import SyntheticImgCptDataset
    from magma_amd.train_engine import initialize
    from magma_amd.utils import cycle
    cfg = model.config
    cfg.gradient_accumulation_steps, cfg.batch_size = 1, 2
    ds = SyntheticImgCptDataset(8, image_size=64, seq_len=model.seq_len, eos=model.eos_token, vocab=1000, seed=3)
    engine, _, loader, _ = initialize(model, cfg, training_data=ds)
    return engine, cycle(loader), cfg


def inputs(seed=5):
    """Two images and one token per row: with the 4-position image prefix a prompt of 5 rows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 64, 64, generator=g).to(BF16).float(), torch.randint(0, 1000, (2, 1), generator=g)


def lm_inputs(model, S=5, seed=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, S, model.lm.config.hidden_size, generator=g).to(BF16).to(model.device)


class Trace(NamedTuple):
    emb: torch.Tensor      # what Magma.embed made of the inputs (encoder, prefix projection, word embeddings)
    logits: list           # fp32 logits of the prefill and of every token step
    tokens: torch.Tensor   # of the public generate()
    cache: object          # the pooled cache both ran on


GREEDY = dict(max_steps=STEPS, temperature=0.0, decode=False, stop_on_eos=False)


@torch.no_grad()
def drive(model, images=None, ids=None, emb=None) -> Trace:
    """Prefill on the pooled cache and STEPS token steps with decode()'s default use_graph (eager, capture, replay, replay), each fed
    the argmax of the logits before it; then the public greedy generate() on the same shapes, i.e. on the same pooled cache.
    The prefill arms the cache with the eos id generate() arms it with: a change of that id drops the cache's graphs
    (_arm_first_token), and the steps captured here are to survive the generate() call, up to the next drive."""
    eng = model.lm.engine
    if emb is None:
        emb = model.embed([images, ids])
    o = eng.forward(inputs_embeds=emb, use_cache=True, reuse_cache=True, cache_hint=STEPS, eos_token=model.eos_token)
    cache = o.past_key_values
    logits = [o.logits[:, -1].float().clone()]
    for _ in range(STEPS):
        lg, _ = eng.decode(logits[-1].argmax(-1, keepdim=True), cache)
        logits.append(lg.float().clone())
    tokens = model.generate(emb, **GREEDY).clone()
    assert list(eng._cache_pool.values()) == [cache], "generate() did not run on the drive's pooled cache"
    assert len(cache.decode_state.graphs) >= 2, "the drive's step and generate()'s are not both captured: nothing stale could be replayed"
    return Trace(emb.clone(), logits, tokens, cache)


def assert_same(warm: Trace, cold: Trace, what: str):
    assert torch.equal(warm.emb, cold.emb), f"{what}: Magma.embed differs from the cold model's"
    for i, (a, b) in enumerate(zip(warm.logits, cold.logits)):
        assert torch.equal(a, b), (f"{what}: logits of {'the prefill' if i == 0 else f'token step {i}'} differ from the cold model's: "
                                   f"max |diff| {float((a - b).abs().max()):.3e} of max |logit| {float(b.abs().max()):.3e}")
    assert torch.equal(warm.tokens, cold.tokens), (what, warm.tokens, cold.tokens)


def assert_moved(before: Trace, after: Trace, what: str):
    """The write matters: measured on cold models only, the logits of every compared step differ."""
    for i, (a, b) in enumerate(zip(before.logits, after.logits)):
        assert not torch.equal(a, b), f"{what}: the write left the logits of step {i} as they were: the comparison would pass vacuously"


def has_derived(model, case) -> bool:
    """The derived operand the case is about exists on the engine's first layer (a dict of copies: is not empty)."""
    obj = model.lm.engine.layers[0]
    for name in CASES[case][3]:
        obj = getattr(obj, name)
    return obj is not None and (not isinstance(obj, dict) or len(obj) > 0)


def clone_cache(cache):
    """The cache's rows and positions on fresh buffers, WITHOUT its decode state (scratch, plan, captured steps)."""
    from magma_amd.engine import KVCache
    L, B, H, Smax, _ = cache.k.shape
    c = KVCache(L, B, H, Smax, cache.k.device, ragged=cache.ragged)
    for name in ("k", "v", "d_pos", "sample_state", "seed", "history"):
        getattr(c, name).copy_(getattr(cache, name))
    c.pos, c.eos, c._rows_at = cache.pos, cache.eos, cache._rows_at
    c._rows = None if cache._rows is None else cache._rows.clone()
    c.pending = None if cache.pending is None else cache.pending.clone()
    return c


# ------------------------------------------------------------------------------------------------------ the fp32 oracle
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def anchor(cold, case, trace: Trace, images, ids):
    """oracle.model.magma_forward at the cold model's parameters against the cold prefill logits, under the rule of
    tests/test_model_gpu.py: err(HIP, fp32 oracle) <= 2 err(the oracle run in bf16, fp32 oracle) + 2e-3."""
    from oracle.model import OracleConfig, magma_forward
    cfg = OracleConfig.tiny(n_positions=128, eos_token=cold.eos_token, image_token=cold.image_token, **CASES[case][2])
    p = {k: v.detach().float().cpu() for k, v in cold.state_dict().items()}
    pb = {k: (v.to(BF16) if v.is_floating_point() else v) for k, v in p.items()}
    P = trace.emb.shape[1] - ids.shape[1]
    caps = torch.cat([ids, torch.full((ids.shape[0], P), cold.eos_token, dtype=torch.int64)], dim=1)     # (B, P + 1): P + 1 rows
    with torch.no_grad():
        ref = magma_forward(p, cfg, images, caps)["logits"][:, -1]
        bf = magma_forward(pb, cfg, images.to(BF16), caps)["logits"][:, -1]
    e_hip, e_bf = rel(trace.logits[0], ref), rel(bf, ref)
    print(f"[lifecycle] {case}: cold prefill logits against the fp32 oracle {e_hip:.3e}, the oracle in bf16 {e_bf:.3e}")
    assert ref.shape == trace.logits[0].shape
    assert e_hip <= 2.0 * e_bf + 2e-3, f"{case}: HIP err {e_hip:.3e} vs eager-bf16 err {e_bf:.3e}"
