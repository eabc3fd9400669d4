"""Inputs of the parity cases against the reference's own code (tests/test_host_cpu.py, tests/test_oracle_pins.py): the same
on-disk dataset, toy models, stand-in `self` objects, recording engines and loader are handed to the reference's functions by
tests/golden/make_host_golden.py, which stores what they returned in tests/golden/reference_host_pins.pt, and to this repo's
functions (or the oracle) by the tests, which compare against it."""
import json
from types import SimpleNamespace

import numpy as np
import torch

CONFIG_FIELDS = ("encoder_name", "adapter_config", "lr", "image_enc_lr", "batch_size", "gradient_accumulation_steps",
                 "use_image_embed_layernorm", "image_embed_dropout_prob", "image_size", "gradient_clipping")
V2_EXTRA_KEYS = ("dataset_type", "vqa_dir", "gqa_dir")      # in the published MAGMA_v2.yml, not fields of the reference class

PARAM_GROUP_CASES = [(0.0, 2e-6, True), (0.05, 2e-6, True), (0.05, None, False), (0.0, 2e-6, False)]
DATASET_SEQ_LEN, DATASET_IMAGE_SIZE, COLLATE_SEQ_LEN = 40, 32, 24


def write_dataset(root):
    """Two shards in the reference's on-disk layout: a record without image_path (path inferred from the record's name),
    greyscale and RGB images, single-caption records."""
    import PIL.Image as I
    rng = np.random.RandomState(1)
    n = 0
    for shard in ("00000", "00001"):
        (root / "image_data" / shard).mkdir(parents=True)
        (root / "images" / shard).mkdir(parents=True)
        for i in range(4):
            grey = (i == 2)
            arr = (rng.rand(37 + i, 61) * 255).astype("uint8") if grey else (rng.rand(37 + i, 61, 3) * 255).astype("uint8")
            I.fromarray(arr).save(root / "images" / shard / f"{i}.jpg")
            rec = {"captions": [f"a caption for image {shard}/{i}, long enough to be cut"], "metadata": {"n": n}}
            if i != 1:
                rec["image_path"] = f"images/{shard}/{i}.jpg"
            (root / "image_data" / shard / f"{i}.json").write_text(json.dumps(rec))
            n += 1


def dataset_tokenizer_and_transform():
    from magma_amd.tokenizer import ByteTokenizer
    from magma_amd.transforms import clip_preprocess
    return ByteTokenizer(DATASET_SEQ_LEN), clip_preprocess(DATASET_IMAGE_SIZE)


def param_group_model(use_ln):
    """A model with the reference's attribute structure (image_prefix.enc / .proj / .ln, lm with Embedding / LayerNorm / Linear
    + frozen tensors)."""
    nn = torch.nn
    torch.manual_seed(0)
    model = nn.Module()
    model.image_prefix = nn.Module()
    model.image_prefix.enc = nn.Sequential(nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4), nn.Conv2d(4, 4, 1))
    model.image_prefix.proj = nn.Linear(4, 8)
    if use_ln:
        model.image_prefix.ln = nn.LayerNorm(8)
    model.lm = nn.Sequential(nn.Embedding(11, 8), nn.LayerNorm(8), nn.Linear(8, 8), nn.Sequential(nn.Linear(8, 2), nn.ReLU(), nn.Linear(2, 8)),
                             nn.Linear(8, 11))
    for p in list(model.lm[0].parameters()) + list(model.lm[2].parameters()) + list(model.lm[4].parameters()):
        p.requires_grad_(False)                       # frozen LM, trainable adapters + LayerNorm
    return model


def param_group_config(weight_decay, image_enc_lr, use_ln):
    sched = {"scheduler": {"type": "WarmupDecayLR", "params": {"warmup_min_lr": 0, "warmup_max_lr": 8e-4}}}
    return SimpleNamespace(weight_decay=weight_decay, image_enc_lr=image_enc_lr, use_image_embed_layernorm=use_ln, lr=8e-4, min_lr=1e-7,
                           deepspeed_config_params=sched)


def describe_param_groups(model, groups):
    """Groups as data: (lr, weight_decay, parameter names in order) per group."""
    names = {id(p): n for n, p in model.named_parameters()}
    return [(g.get("lr"), g.get("weight_decay"), [names[id(p)] for p in g["params"]]) for g in groups]


class RecordingEngine:
    """Records the calls train_step / eval_step make: forward (image shape, images all zero, captions), backward (loss), step."""
    device = torch.device("cpu")

    def __init__(self):
        self.events, self.n = [], 0

    def __call__(self, images, captions, **kw):
        self.n += 1
        self.events.append(("forward", tuple(images.shape), float(images.float().abs().sum()) == 0.0, captions.clone()))
        return SimpleNamespace(loss=torch.tensor(float(self.n) * 0.5))

    def backward(self, loss):
        self.events.append(("backward", float(loss)))

    def step(self):
        self.events.append(("step",))


def step_loader():
    g = torch.Generator().manual_seed(3)
    while True:
        yield torch.rand(2, 3, 8, 8, generator=g) + 0.1, torch.randint(0, 50, (2, 16), generator=g)


def step_config(run_blind):
    return SimpleNamespace(gradient_accumulation_steps=3, eval_steps=2, run_blind=run_blind)


class CheckpointEngine:
    def __init__(self, ok=True):
        self.saved, self.ok = [], ok

    def save_checkpoint(self, save_dir, client_state=None, tag=None):
        self.saved.append((str(save_dir), client_state))

    def load_checkpoint(self, load_dir, load_optimizer_states=True, load_lr_scheduler_states=True, tag=None):
        if not self.ok:
            raise AssertionError("no checkpoint here")
        return str(load_dir), {"global_step": 1234}


def checkpoint_config():
    return SimpleNamespace(to_dict=lambda: {"lr": 8e-4, "encoder_name": "clip_resnet_large", "nested": {"a": [1, 2]}})


def checkpoint_helpers_run(save_model, load_model, infer_checkpoint_path_from_config, tmp_path):
    """save_model / load_model / infer_checkpoint_path_from_config on a recording engine and a directory tree built up in three
    stages (nothing; a `latest` tag; the tagged folder with the model file), as data: paths under tmp_path written as <tmp>."""
    def rel(x):
        return x.replace(str(tmp_path), "<tmp>") if isinstance(x, str) else x

    d = tmp_path / "save"
    e = CheckpointEngine()
    save_model(e, str(d), 77, checkpoint_config())
    out = {"client_state": e.saved[0][1], "config_yml": (d / "config.yml").read_text(),
           "load": [load_model(CheckpointEngine(ok=True), str(d)), load_model(CheckpointEngine(ok=False), str(d)),
                    load_model(CheckpointEngine(ok=True), str(d), load_optimizer_states=False, load_lr_scheduler_states=False)]}
    try:
        infer_checkpoint_path_from_config(SimpleNamespace(save=None))
        out["save_none"] = "returned"
    except ValueError:
        out["save_none"] = "ValueError"
    save = tmp_path / "ckpts"
    stages = []
    for stage in range(3):
        try:
            stages.append(("ok", rel(str(infer_checkpoint_path_from_config(SimpleNamespace(save=str(save)))))))
        except ValueError as ex:
            stages.append(("ValueError", rel(str(ex))))
        if stage == 0:
            save.mkdir()
            (save / "latest").write_text("global_step500\n")
        elif stage == 1:
            (save / "global_step500").mkdir()
            (save / "global_step500" / "mp_rank_00_model_states.pt").write_bytes(b"x")
    out["infer"] = stages
    return out


# ---- tests/test_oracle_pins.py: the reference's Magma / ImagePrefix methods around the oracle's pieces

def plumbing_inputs():
    """Oracle parameters and one batch for Magma.forward / Magma.embed: images, eos-padded captions of two lengths, a token run."""
    import oracle.model as om
    cfg = om.OracleConfig.tiny(n_positions=64)
    p = om.init_params(cfg, seed=5)
    g = torch.Generator().manual_seed(11)
    B = 2
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = torch.full((B, 64), cfg.eos_token, dtype=torch.int64)
    caps[0, :13] = torch.randint(0, 1000, (13,), generator=g)
    caps[1, :5] = torch.randint(0, 1000, (5,), generator=g)
    toks = torch.randint(0, 1000, (B, 7), generator=g)
    return cfg, p, images, caps, toks


ADD_ADAPTER_CASES = [(t, kw) for kw in ({}, {"add_layernorm": True}, {"downsample_factor": 8})
                     for t in ("normal", "parallel", "scaled_parallel")]


def adapter_case_key(adapter_type, kwargs):
    return adapter_type, tuple(sorted(kwargs.items()))


def adapter_toy():
    """A stand-in `self` for Magma.add_adapters: a ModuleList of blocks with .attn / .mlp."""
    import torch.nn as nn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = nn.Linear(16, 16, bias=False)
            self.mlp = nn.Sequential(nn.Linear(16, 64), nn.Linear(64, 16))

    tr = nn.ModuleList([Block() for _ in range(3)])
    return SimpleNamespace(transformer=tr, mlp_adapter_added=False, attn_adapter_added=False, device=torch.device("cpu"),
                           dtype=torch.float32, lm=SimpleNamespace(config=SimpleNamespace(hidden_size=16), invalidate_packed=lambda: None))


def add_adapters_run(add_adapters, obj, adapter_type, kwargs):
    """Both locations, then a second call at the same location: parameter names -> shapes, the flags, what the second call raised."""
    for location in ("mlp", "attention"):
        add_adapters(obj, adapter_type=adapter_type, location=location, **kwargs)
    shapes = {n: tuple(p.shape) for n, p in obj.transformer.named_parameters()}
    try:
        add_adapters(obj, adapter_type=adapter_type, location="mlp")
        again = None
    except Exception as e:  # noqa: BLE001
        again = type(e).__name__
    return {"shapes": shapes, "added": (obj.mlp_adapter_added, obj.attn_adapter_added), "second_call_raises": again}


PREPROCESS_PROMPT = "Describe the painting:"


def preprocess_image(root):
    import PIL.Image as I
    path = str(root / "img.png")
    I.fromarray((np.random.RandomState(0).rand(45, 70, 3) * 255).astype("uint8")).save(path)
    return path


def preprocess_stand_in(tag, seen):
    """A stand-in `self` for Magma.preprocess_inputs: this repo's tokenizer and transform, an embed that records its list."""
    from magma_amd.tokenizer import ByteTokenizer
    from magma_amd.transforms import clip_preprocess

    def embed(lst):
        seen[tag] = [t.clone() for t in lst]
        return "embedded"
    return SimpleNamespace(tokenizer=ByteTokenizer(64), transforms=clip_preprocess(32), embed=embed)


def image_prefix_inputs():
    """Oracle parameters and images for ImagePrefix.forward on a sequence encoder; operands of the pooled-encoder branch."""
    import oracle.model as om
    cfg = om.OracleConfig.tiny()
    p = om.init_params(cfg, seed=9)
    images = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    C, S, d = 24, 3, 16
    g = torch.Generator().manual_seed(4)
    pp = {"image_prefix.proj.weight": torch.randn(S * d, C, generator=g) * 0.1, "image_prefix.proj.bias": torch.randn(S * d, generator=g) * 0.1,
          "image_prefix.ln.weight": torch.rand(d, generator=g) + 0.5, "image_prefix.ln.bias": torch.randn(d, generator=g) * 0.1}
    feats = torch.randn(2, C, generator=g)
    return cfg, p, images, (C, S, d, pp, feats)
