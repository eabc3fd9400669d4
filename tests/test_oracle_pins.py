"""Pins the oracle (and the host-side sampling logic) to outputs of the
reference's own code, captured by tests/golden/make_golden.py (which ran the
reference's magma/{adapters,sampling,utils}.py in place) and by
tests/golden/make_host_golden.py (its Magma / ImagePrefix methods).  CPU only."""
import os
import sys
import types

import pytest

import torch

from oracle import model as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_cases as RC  # noqa: E402

# what the reference's own code returned, run in place by tests/golden/make_host_golden.py on the inputs of tests/reference_cases.py
HOST_PINS = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_host_pins.pt"), weights_only=False)

PINS = torch.load(os.path.join(os.path.dirname(__file__), "golden", "reference_pins.pt"), weights_only=False)


def test_adapter_matches_reference():
    pin = PINS["adapter"]
    p = {"a." + k.replace("adapter.", ""): v for k, v in pin["sd"].items()}
    y = O.adapter_fwd(p, "a.", pin["x"])
    assert torch.allclose(y, pin["y"], atol=1e-6, rtol=1e-6)
    assert PINS["adapter_init_absmax"] <= 2e-3 + 1e-9      # reference adapters.py:28-33 clamp
    q = O.init_params(O.OracleConfig.tiny(), 0)
    assert float(q["lm.transformer.h.0.mlp.1.adapter.0.weight"].abs().max()) <= 2e-3 + 1e-9


def test_adapter_wrapper_matches_reference():
    pin = PINS["adapter_wrapper"]
    p = {"a." + k.replace("adapter.", ""): v for k, v in pin["sd"].items() if k.startswith("adapter.")}
    attn_out = pin["x"] * 0.5 + 1.0                     # the toy attention block used by make_golden.py
    assert torch.allclose(O.adapter_fwd(p, "a.", attn_out), pin["y"], atol=1e-6, rtol=1e-6)
    assert pin["rest"] == ["present", "weights"]        # tuple tail is passed through untouched


def test_sampling_filters_match_reference():
    from magma_amd import sampling as S
    for mod in (O, S):
        for thr, key in ((0.9, "out_0.9"), (0.5, "out_0.5")):
            got = mod.top_p_filter(PINS["top_p"]["logits"].clone(), thr)
            assert torch.equal(got, PINS["top_p"][key]), (mod.__name__, thr)
        assert torch.equal(mod.top_k_filter(PINS["top_k"]["logits"].clone(), 5), PINS["top_k"]["out_5"])
    assert S.remove_tokens_after_eos(PINS["remove_eos"]["in"].clone(), 1, 7) == PINS["remove_eos"]["out"]
    assert S.remove_tokens_after_eos(PINS["remove_eos_none"]["in"].clone(), 1, 7) == PINS["remove_eos_none"]["out"]


def test_build_labels_matches_reference():
    pin = PINS["build_labels"]
    got = O.build_labels(pin["P"], pin["captions"], pin["eos"])
    assert torch.equal(got, pin["labels"])


def test_generate_loop_matches_reference():
    """Our sampling.generate driven by the same toy LM must emit the same token
    ids, strings and (prefill, then one-id-per-step) call pattern."""
    from magma_amd import sampling as S
    pin = PINS["generate_toy"]

    class ToyLM:
        def __init__(self, V):
            self.V, self.calls = V, []

        def __call__(self, inputs_embeds=None, input_ids=None, use_cache=None, past_key_values=None, cache_hint=None,
                     reuse_cache=False):
            from magma_amd.language_model import LMOutput
            if inputs_embeds is not None:
                last = (inputs_embeds[:, -1, :].sum(-1) * 7).long() % self.V
                seen = inputs_embeds.shape[1]
            else:
                last, seen = input_ids[:, -1], past_key_values + 1
            self.calls.append(("embeds" if inputs_embeds is not None else "ids", seen))
            idx = torch.arange(self.V)[None, :]
            logits = (-((idx - (last[:, None] * 3 + seen) % self.V) ** 2).float())[:, None, :]
            return LMOutput(logits=logits, past_key_values=seen, next_token=logits[:, -1].argmax(-1))

    class ToyModel:
        training = False

        def __init__(self):
            self.lm = ToyLM(17)
            self.eos_token, self.image_token = 16, 15
            self.device = torch.device("cpu")
            self.tokenizer = types.SimpleNamespace(decode=lambda ids: " ".join(map(str, ids)))

        def eval(self):
            return self

        def train(self, mode=True):
            return self

    tm = ToyModel()
    toks = S.generate(tm, pin["emb"], max_steps=6, temperature=0.0, decode=False)
    assert torch.equal(toks, pin["tokens"])
    assert tm.lm.calls == pin["calls"]
    assert S.generate(ToyModel(), pin["emb"], max_steps=6, temperature=0.0, decode=True) == pin["strings"]


# ---- preprocessing: the third-party arithmetic behind reference transforms.py:121-134 is Pillow's resampler ----
PRE_GEOMS = [(480, 640, 384), (300, 200, 224), (224, 224, 384), (1000, 750, 384), (97, 131, 384), (384, 384, 384),
             (500, 333, 224), (64, 64, 224)]


@pytest.mark.parametrize("H,W,n_px", PRE_GEOMS)
def test_preprocess_matches_pil(H, W, n_px):
    """oracle/preprocess.py (numpy integer restatement of Pillow's ImagingResample) against PIL itself, bit for bit,
    then the whole clip transform against the host pipeline that mirrors the reference (PIL + torch)."""
    import numpy as np
    import PIL.Image as PilImage
    from oracle.preprocess import clip_preprocess_u8, resize_bicubic_u8
    from magma_amd.transforms import clip_preprocess
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    nw, nh = (n_px, int(n_px * H / W)) if W <= H else (int(n_px * W / H), n_px)
    ref = np.asarray(PilImage.fromarray(img).resize((nw, nh), PilImage.BICUBIC))
    assert np.array_equal(resize_bicubic_u8(img, nw, nh), ref)
    host = clip_preprocess(n_px)(PilImage.fromarray(img))[0].numpy()
    assert np.array_equal(clip_preprocess_u8(img, n_px), host)


def test_product_coefficient_tables_equal_oracle():
    """the host half of the device path (magma_amd.transforms.pil_bicubic_tables) builds the same integer tables"""
    import numpy as np
    from oracle.preprocess import precompute_coeffs
    from magma_amd.transforms import pil_bicubic_tables
    for a, b in [(640, 512), (200, 224), (750, 288), (131, 384), (1000, 384), (333, 224), (64, 224), (4000, 384)]:
        kk, bounds = pil_bicubic_tables(a, b)
        rk, rb = precompute_coeffs(a, b)
        assert np.array_equal(kk.astype(np.int64), rk) and np.array_equal(bounds.astype(np.int64), rb)


def test_parallel_adapters_match_reference():
    """ParallelAdapter / ParallelAdapterWrapper (reference magma/adapters.py:42-92), run in place by make_golden.py
    around a toy wrapped module: y = module(x) + adapter(x) * adapter_scale."""
    for key, module_out in (("parallel_adapter", lambda x: torch.tanh(x) * 2.0 - 0.25),
                            ("parallel_adapter_scaled", lambda x: torch.tanh(x) * 2.0 - 0.25),
                            ("parallel_adapter_wrapper", lambda x: x * 0.5 + 1.0)):
        pin = PINS[key]
        p = {"a." + k.replace("adapter.", ""): v for k, v in pin["sd"].items() if k.startswith("adapter.")}
        if "adapter_scale" in pin["sd"]:
            p["scale"] = pin["sd"]["adapter_scale"]
        y = O.parallel_adapter_fwd(p, "a.", "scale", pin["x"], module_out(pin["x"]))
        assert torch.allclose(y, pin["y"], atol=1e-6, rtol=1e-6), key
    assert "adapter_scale" not in PINS["parallel_adapter"]["sd"]          # plain "parallel": the scale is the constant 1
    assert float(PINS["parallel_adapter_scaled"]["sd"]["adapter_scale"]) == 1.75
    assert PINS["parallel_adapter_wrapper"]["rest"] == ["present", "weights"]


@pytest.mark.parametrize("name,act", [("gelu", "gelu"), ("gelu_tanh", "gelu_tanh"), ("ln", "relu"), ("ln_gelu", "gelu")])
def test_adapter_options_match_reference(name, act):
    """reference adapters.py:11-24: ``activation`` and ``add_layernorm`` -- the reference's own Adapter run in place with each
    option (tests/golden/make_golden.py), against the oracle's statement of it; and the product module builds the same
    state-dict keys for every option set."""
    import functools
    pin = PINS["adapter_options"][name]
    p = {"a." + k.replace("adapter.", ""): v for k, v in pin["sd"].items()}
    y = O.adapter_fwd(p, "a.", pin["x"], act)
    assert torch.allclose(y, pin["y"], atol=2e-6, rtol=1e-5)
    from magma_amd.adapters import Adapter
    kw = {"gelu": dict(activation=torch.nn.GELU), "gelu_tanh": dict(activation=functools.partial(torch.nn.GELU, approximate="tanh")),
          "ln": dict(add_layernorm=True), "ln_gelu": dict(add_layernorm=True, activation=torch.nn.GELU)}[name]
    mod = Adapter(dim=64, downsample_factor=4, **kw)
    assert set(mod.state_dict()) == set(pin["sd"])
    assert (mod.ln is not None) == name.startswith("ln") and mod.down.weight.shape == (16, 64) and mod.up.weight.shape == (64, 16)
    assert not mod.plain
    with pytest.raises(NotImplementedError):
        Adapter(dim=64, activation=torch.nn.Tanh)


def test_oracle_forward_and_embed_plumbing_equal_the_reference_methods_run_in_place(monkeypatch):
    """reference magma/magma.py:195-212 (Magma.embed) and :238-276 (Magma.forward): the two method bodies, extracted with ast and executed
    IN PLACE by tests/golden/make_host_golden.py on a stand-in `self` whose image_prefix / word_embedding are the oracle's pieces and whose
    `lm` records what it is handed -- together with the reference's own build_labels (utils.py:334-364).  What the reference handed its
    LM (inputs_embeds: prefix, then the caption embeddings cut so that the total is seq_len; labels) is exactly what
    oracle.magma_forward hands oracle.lm_forward, and oracle.embed equals the reference's embed on a [image, tokens, image] list.  The
    oracle is given the image prefixes the reference's stand-in computed (pinned with it; this machine's own prefix agrees to fp32
    rounding), so the comparison stays exact.  This pins the PLUMBING of a3 / a11 (concat order, truncation, label construction); the
    arithmetic of the pieces is pinned elsewhere."""
    import oracle.model as om
    pin = HOST_PINS["plumbing"]
    cfg, p, images, caps, toks = RC.plumbing_inputs()
    assert torch.allclose(om.image_prefix_fwd(p, cfg, images), pin["forward_prefix"], atol=1e-4, rtol=1e-4)
    assert pin["forward_returns"] == "lm-output" and pin["forward_prefix_got_images"]
    handed, prefixes = {}, []

    def pinned_prefix(p_, cfg_, x, *a, **k):
        prefixes.append(x.clone())
        return queue.pop(0)

    def record(p_, cfg_, inputs_embeds=None, labels=None, **kw):
        handed["oracle"] = (inputs_embeds.clone(), labels.clone())
        return {"loss": torch.zeros(()), "logits": None}
    monkeypatch.setattr(om, "image_prefix_fwd", pinned_prefix)
    monkeypatch.setattr(om, "lm_forward", record)
    queue = [pin["forward_prefix"]]
    om.magma_forward(p, cfg, images, caps)
    assert len(prefixes) == 1 and torch.equal(prefixes[0], images)
    assert torch.equal(pin["forward_labels"], handed["oracle"][1])                 # labels: integer, exact
    assert pin["forward_embeds"].shape == handed["oracle"][0].shape == (images.shape[0], 64, cfg.d_model)
    assert torch.equal(pin["forward_embeds"], handed["oracle"][0])
    assert pin["short_captions_raise"] == "AssertionError"                        # captions must be padded to seq_len
    # embed: [image, tokens, image] (the reference casts images with .half(): the stand-in prefix takes them back to fp32)
    queue, prefixes = list(pin["embed_prefixes"]), []
    assert pin["embed_prefix_got_half_images"] == [True, True]
    mine = om.embed(p, cfg, [images.half().float(), toks, images.half().float()])
    assert len(prefixes) == 2 and all(torch.equal(x, images.half().float()) for x in prefixes)
    assert torch.allclose(pin["embed"], mine, atol=0, rtol=0)
    assert pin["embed_bad_input_raises"] == "ValueError"


@pytest.mark.parametrize("adapter_type", ["normal", "parallel", "scaled_parallel"])
@pytest.mark.parametrize("kwargs", [{}, {"add_layernorm": True}, {"downsample_factor": 8}])
def test_add_adapters_builds_the_reference_module_tree(adapter_type, kwargs):
    """reference magma/magma.py:102-174 (Magma.add_adapters), the method body extracted with ast and executed IN PLACE by
    tests/golden/make_host_golden.py with the reference's own adapter classes (magma/adapters.py imported in place) on a toy `self`
    (ModuleList of blocks with .attn / .mlp), next to this repo's Magma.add_adapters on an identical toy: the same parameter names --
    the checkpoint keys of SURVEY Q8 -- with the same shapes for every adapter type at both locations and with the reference's
    options; a second call at the same location raises on both."""
    from magma_amd.magma import Magma
    pin = HOST_PINS["add_adapters"][RC.adapter_case_key(adapter_type, kwargs)]
    mine = RC.add_adapters_run(Magma.add_adapters, RC.adapter_toy(), adapter_type, kwargs)
    assert pin["shapes"] == mine["shapes"] and len(pin["shapes"]) > 3 * 3
    assert pin["added"] == mine["added"] == (True, True)
    assert pin["second_call_raises"] == mine["second_call_raises"] == "ValueError"


def test_preprocess_inputs_equals_the_reference_method_run_in_place(tmp_path):
    """reference magma/magma.py:176-193 (Magma.preprocess_inputs) with the reference's own ImageInput (magma/image_input.py:6-23), both
    executed IN PLACE by tests/golden/make_host_golden.py, next to this repo's method and ImageInput on the same stand-in `self` (same
    tokenizer, same transform, an embed that records): the caller's list is mutated to the same tensors (token ids (1, T) int64, image
    (1, 3, n, n)), embed is handed the same list, embed=False returns the list itself, an unknown item type raises."""
    from magma_amd.image_input import ImageInput
    from magma_amd.magma import Magma
    pin = HOST_PINS["preprocess_inputs"]
    path = RC.preprocess_image(tmp_path)
    seen = {}
    l_mine = [ImageInput(path), RC.PREPROCESS_PROMPT, ImageInput(path)]
    assert pin["returns"] == "embedded" and Magma.preprocess_inputs(RC.preprocess_stand_in("mine", seen), l_mine) == "embedded"
    assert len(pin["list"]) == len(l_mine) == 3
    for a, b, c, d in zip(pin["list"], l_mine, pin["embedded"], seen["mine"]):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b) and torch.equal(c, d) and torch.equal(a, c)
    assert l_mine[0].shape == (1, 3, 32, 32) and l_mine[1].dtype == torch.int64 and l_mine[1].shape[0] == 1
    keep_mine = ["x"]
    assert pin["embed_false_returns_list"] and Magma.preprocess_inputs(RC.preprocess_stand_in("m", {}), keep_mine, embed=False) is keep_mine
    assert "Invalid input type" in pin["invalid_raises"][1]
    with pytest.raises(Exception, match="Invalid input type"):
        Magma.preprocess_inputs(RC.preprocess_stand_in("mine", {}), [3.14])


def test_oracle_image_prefix_plumbing_equals_the_reference_method_run_in_place(monkeypatch):
    """reference magma/image_prefix.py:78-109 (ImagePrefix.forward) extracted with ast and executed IN PLACE by
    tests/golden/make_host_golden.py (with the file's own ENCODER_SEQ_LENS table and einops.rearrange) on a stand-in `self` whose
    encoder / Linear / LayerNorm carry the oracle's tensors: (a) sequence encoders (clip_resnet_large: features (B, HW, C), no reshape)
    == oracle.image_prefix_fwd, given the encoder features the reference's stand-in computed (pinned with it; this machine's own
    features agree to fp32 rounding); (b) pooled encoders (features (B, C, 1, 1) -> Linear to seq*d -> "b (s d) -> b s d") ==
    oracle.pooled_prefix_fwd."""
    import oracle.model as om
    pin = HOST_PINS["image_prefix"]
    assert pin["seq_len_clip_resnet_large"] == 144
    cfg, p, images, (C, S, d, pp, feats) = RC.image_prefix_inputs()
    assert pin["encoder_got_images"]
    assert torch.allclose(om.encoder_fwd(p, cfg, images), pin["encoder_out"], atol=1e-4, rtol=1e-4)
    seen = []

    def pinned_encoder(p_, cfg_, x, *a, **k):
        seen.append(x.clone())
        return pin["encoder_out"].clone()
    monkeypatch.setattr(om, "encoder_fwd", pinned_encoder)
    got = pin["sequence"]
    with torch.no_grad():
        want = om.image_prefix_fwd(p, cfg, images)
    assert len(seen) == 1 and torch.equal(seen[0], images)
    assert got.shape == want.shape and got.ndim == 3 and torch.allclose(got, want, atol=1e-6, rtol=1e-6)
    # pooled encoder: (B, C, 1, 1) features, out_seq_len tokens from one Linear
    with torch.no_grad():
        got2, want2 = pin["pooled"], om.pooled_prefix_fwd(pp, d, S, feats)
    assert got2.shape == (2, S, d) and torch.allclose(got2, want2, atol=1e-6, rtol=1e-6)


def test_oracle_window_is_exact():
    """tests/fullwidth_common.oracle_window: the S = 2048 GPU parity tests evaluate the CPU oracle on the first
    ceil64(P + longest caption + 2) positions only.  Loss, labels, target-row logits and every gradient must be the values of the
    full-length evaluation (causal mask: no position influences an earlier one; build_labels masks everything behind the first
    eos, reference magma/utils.py:334-364) -- checked here on the tiny configuration, full length 256 against the window."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fullwidth_common as F
    cfg = O.OracleConfig.tiny(n_positions=256)
    params = O.init_params(cfg, seed=3)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    g = torch.Generator().manual_seed(2)
    B, S, P = 2, 256, 4
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :37] = torch.randint(0, 1000, (37,), generator=g)
    caps[1, :9] = torch.randint(0, 1000, (9,), generator=g)
    mask = (torch.rand(B, P, cfg.d_model, generator=g) < 0.9).float() / 0.9
    win = F.oracle_window(caps, P, cfg.eos_token)
    assert win.shape == (B, 64) and torch.equal(win, caps[:, :64])
    names = [k for k in params if (".adapter." in k or k.startswith("image_prefix.")) and "running_" not in k]

    def run(c):
        p = {k: (v.detach().clone() if v.is_floating_point() else v) for k, v in params.items()}
        for k in names:
            p[k].requires_grad_(True)
        out = O.magma_forward(p, cfg, images, c, dropout_mask=mask)
        out["loss"].backward()
        return out, {k: p[k].grad for k in names}

    full, g_full = run(caps)
    part, g_part = run(win)
    assert torch.equal(full["labels"][:, :64], part["labels"]) and bool((full["labels"][:, 64:] == -100).all())
    assert abs(float(full["loss"]) - float(part["loss"])) <= 1e-6 * abs(float(full["loss"]))
    rows = (part["labels"][0, 1:] != -100).nonzero().squeeze(1)
    assert torch.allclose(full["logits"][0, rows], part["logits"][0, rows], rtol=1e-5, atol=1e-5)
    for k in names:
        a, b = g_full[k], g_part[k]
        assert float((a - b).norm()) <= 1e-5 * float(a.norm()) + 1e-12, k
