"""Generates tests/golden/reference_host_pins.pt by RUNNING the reference's own host-side code in place (read-only, nothing
copied) on the inputs of tests/reference_cases.py, for tests/test_host_cpu.py and tests/test_oracle_pins.py:

  * magma/config.py (MultimodalConfig + the derived DeepSpeed dictionary) on the published configs/MAGMA_v1.yml / MAGMA_v2.yml,
    which are copied to tests/golden/reference_configs/ as test data;
  * magma/datasets/dataset.py (ImgCptDataset, collate_fn) on a two-shard on-disk dataset;
  * from magma/utils.py, extracted with ``ast`` (the module itself needs deepspeed / wandb / gdown):
    get_params_for_weight_decay_optimization + configure_param_groups, reduce_losses, save_model / load_model /
    infer_checkpoint_path_from_config;
  * magma/train_loop.py (train_step / eval_step) against a recording engine;
  * from magma/magma.py, extracted with ``ast``: Magma.forward / Magma.embed (with utils.py's build_labels) around the oracle's
    image prefix and word embedding, Magma.add_adapters with the reference's adapters.py, Magma.preprocess_inputs with the
    reference's image_input.py; from magma/image_prefix.py: ImagePrefix.forward around the oracle's encoder and weights.

An annotation-only ``torchtyping`` shim stands in for the one missing dependency.  Re-run:
    python tests/golden/make_host_golden.py <path to a checkout of the reference MAGMA repository>
"""
import ast
import copy
import dataclasses
import importlib.util
import os
import shutil
import sys
import tempfile
import types
from collections import defaultdict
from pathlib import Path

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import reference_cases as C  # noqa: E402

OUT = os.path.join(HERE, "reference_host_pins.pt")
CONFIGS = os.path.join(HERE, "reference_configs")       # the published YAMLs, kept as data for the parser tests


def _shim_torchtyping():
    tt = types.ModuleType("torchtyping")

    class TensorType:
        def __class_getitem__(cls, item):
            return cls
    tt.TensorType, tt.patch_typeguard = TensorType, (lambda: None)
    sys.modules.setdefault("torchtyping", tt)


def _module(ref, name, rel, stubs=None):
    """One reference source file executed in place as module refmagma.<name>, stub siblings for its relative imports."""
    pkg = sys.modules.setdefault("refmagma", types.ModuleType("refmagma"))
    pkg.__path__ = []
    for sname, attrs in (stubs or {}).items():
        m = types.ModuleType(f"refmagma.{sname}")
        m.__dict__.update(attrs)
        sys.modules[f"refmagma.{sname}"] = m
    spec = importlib.util.spec_from_file_location(f"refmagma.{name}", os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "refmagma"
    sys.modules[f"refmagma.{name}"] = mod
    spec.loader.exec_module(mod)
    return mod


def _functions(ref, rel, names, ns):
    path = os.path.join(ref, rel)
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns


def config_pins(ref):
    import yaml
    os.makedirs(CONFIGS, exist_ok=True)
    for f in ("MAGMA_v1.yml", "MAGMA_v2.yml"):
        shutil.copyfile(os.path.join(ref, "configs", f), os.path.join(CONFIGS, f))
    m = _module(ref, "config", "magma/config.py", stubs={"utils": {"is_main": lambda: False}})
    r1 = m.MultimodalConfig.from_yml(os.path.join(ref, "configs", "MAGMA_v1.yml"))
    v2 = os.path.join(ref, "configs", "MAGMA_v2.yml")
    try:
        m.MultimodalConfig.from_yml(v2)
        v2_rejected = None
    except TypeError as e:
        v2_rejected = type(e).__name__
    raw = yaml.safe_load(open(v2))
    extra = {k: raw.pop(k) for k in C.V2_EXTRA_KEYS}
    r2 = m.MultimodalConfig(**raw)
    return {"v1": dataclasses.asdict(r1), "v1_deepspeed": r1.deepspeed_config_params,
            "v2": dataclasses.asdict(r2), "v2_deepspeed": r2.deepspeed_config_params, "v2_extra": extra,
            "v2_from_yml_raises": v2_rejected}


def dataset_pins(ref):
    m = _module(ref, "dataset", "magma/datasets/dataset.py")
    tok, tf = C.dataset_tokenizer_and_transform()
    with tempfile.TemporaryDirectory() as d:
        root = Path(d)
        C.write_dataset(root)
        ds = m.ImgCptDataset(root, tok, tf, seq_len=C.DATASET_SEQ_LEN)
        items = [ds[i] for i in range(len(ds))]
        batch = m.collate_fn(items, seq_len=C.COLLATE_SEQ_LEN)
    return {"items": [(im.clone(), cap.clone()) for im, cap in items], "collate": (batch[0].clone(), batch[1].clone())}


def param_group_pins(ref):
    ns = _functions(ref, "magma/utils.py", ("get_params_for_weight_decay_optimization", "configure_param_groups"),
                    {"torch": torch, "defaultdict": defaultdict})
    out = {}
    for case in C.PARAM_GROUP_CASES:
        wd, enc_lr, use_ln = case
        model = C.param_group_model(use_ln)
        cfg = C.param_group_config(wd, enc_lr, use_ln)
        groups = ns["configure_param_groups"](model, cfg)
        out[case] = {"groups": C.describe_param_groups(model, groups), "deepspeed": copy.deepcopy(cfg.deepspeed_config_params)}
    return out


def step_pins(ref):
    import torch.distributed as dist
    ns = _functions(ref, "magma/utils.py", ("reduce_losses",), {"torch": torch, "dist": dist})
    tv, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")
    tvu.make_grid = lambda *a, **k: None
    tv.utils = tvu
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.utils", tvu)
    m = _module(ref, "train_loop", "magma/train_loop.py",
                stubs={"utils": {"reduce_losses": ns["reduce_losses"], "to_cuda_half": lambda *a: a}})
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self        # the reference moves its batch with .half().cuda(): kept on the host
    try:
        out = {}
        for run_blind in (False, True):
            for name, fn in (("train_step", m.train_step), ("eval_step", m.eval_step)):
                e = C.RecordingEngine()
                loss = fn(C.step_config(run_blind), C.step_loader(), e)
                out[(run_blind, name)] = {"loss": float(loss), "events": e.events}
    finally:
        torch.Tensor.cuda = cuda
    return out


def checkpoint_pins(ref):
    import yaml
    ns = _functions(ref, "magma/utils.py", ("save_model", "load_model", "infer_checkpoint_path_from_config"),
                    {"os": os, "Path": Path, "yaml": yaml})
    with tempfile.TemporaryDirectory() as d:
        return C.checkpoint_helpers_run(ns["save_model"], ns["load_model"], ns["infer_checkpoint_path_from_config"], Path(d))


def _methods(ref, rel, cls, names, ns, strip_decorators=False):
    """Method bodies of class `cls` in a reference file, extracted with ast and executed in place as plain functions."""
    path = os.path.join(ref, rel)
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for item in node.body:
                if isinstance(item, ast.FunctionDef) and item.name in names:
                    if strip_decorators:
                        item.decorator_list = []
                    exec(compile(ast.Module(body=[item], type_ignores=[]), path, "exec"), ns)
    return ns


def _raises(fn, *a, **k):
    try:
        fn(*a, **k)
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, str(e)
    return None, None


def plumbing_pins(ref):
    """Magma.forward / Magma.embed (magma.py:195-276) + build_labels (utils.py:334-364) on a stand-in `self` whose image prefix and
    word embedding are the oracle's: what the LM is handed, and the image prefixes the stand-in returned on the way."""
    from typing import List, Optional
    import torch.nn.functional as F
    import oracle.model as om
    ns = {"torch": torch, "TensorType": sys.modules["torchtyping"].TensorType, "List": List, "Optional": Optional, "ModelOutput": object}
    _functions(ref, "magma/utils.py", ("build_labels",), ns)
    _methods(ref, "magma/magma.py", "Magma", ("embed", "forward"), ns, strip_decorators=True)
    cfg, p, images, caps, toks = C.plumbing_inputs()
    handed, prefixes = {}, []

    def image_prefix(x):
        out = om.image_prefix_fwd(p, cfg, x.float())
        prefixes.append((x.float().clone(), out.clone()))
        return out

    def lm(inputs_embeds=None, labels=None, output_hidden_states=False):
        handed["lm"] = (inputs_embeds.clone(), labels.clone())
        return "lm-output"

    fake = types.SimpleNamespace(image_prefix=image_prefix, word_embedding=lambda ids: F.embedding(ids, p["lm.transformer.wte.weight"]),
                                 lm=lm, seq_len=64, eos_token=cfg.eos_token, device=torch.device("cpu"))
    out = {"forward_returns": ns["forward"](fake, images=images, captions=caps)}
    out["forward_embeds"], out["forward_labels"] = handed["lm"]
    x, out["forward_prefix"] = prefixes.pop()
    out["forward_prefix_got_images"] = torch.equal(x, images)
    out["short_captions_raise"] = _raises(ns["forward"], fake, images=images, captions=caps[:, :60])[0]
    prefixes.clear()
    out["embed"] = ns["embed"](fake, [images, toks, images]).clone()
    out["embed_prefix_got_half_images"] = [torch.equal(x, images.half().float()) for x, _ in prefixes]
    out["embed_prefixes"] = [y for _, y in prefixes]
    out["embed_bad_input_raises"] = _raises(ns["embed"], fake, [torch.zeros(3)])[0]
    return out


def add_adapters_pins(ref):
    """Magma.add_adapters (magma.py:102-174) with the reference's adapter classes (adapters.py, imported in place) on a toy `self`."""
    from typing import Literal
    import torch.nn as nn
    ra = _module(ref, "adapters", "magma/adapters.py")
    ns = {"nn": nn, "Literal": Literal, "Adapter": ra.Adapter, "ParallelAdapter": ra.ParallelAdapter,
          "AdapterWrapper": ra.AdapterWrapper, "ParallelAdapterWrapper": ra.ParallelAdapterWrapper}
    _methods(ref, "magma/magma.py", "Magma", ("add_adapters",), ns)
    return {C.adapter_case_key(t, kw): C.add_adapters_run(ns["add_adapters"], C.adapter_toy(), t, kw) for t, kw in C.ADD_ADAPTER_CASES}


def preprocess_inputs_pins(ref):
    """Magma.preprocess_inputs (magma.py:176-193) with the reference's ImageInput (image_input.py:6-23): the caller's list after the call,
    what embed was handed, the list returned under embed=False, the error for an unknown item type."""
    from typing import List
    rii = _module(ref, "image_input", "magma/image_input.py")
    ns = _methods(ref, "magma/magma.py", "Magma", ("preprocess_inputs",), {"torch": torch, "List": List, "ImageInput": rii.ImageInput})
    with tempfile.TemporaryDirectory() as d:
        path = C.preprocess_image(Path(d))
        seen = {}
        lst = [rii.ImageInput(path), C.PREPROCESS_PROMPT, rii.ImageInput(path)]
        ret = ns["preprocess_inputs"](C.preprocess_stand_in("ref", seen), lst)
        keep = ["x"]
        keep_is_returned = ns["preprocess_inputs"](C.preprocess_stand_in("r", {}), keep, embed=False) is keep
    return {"returns": ret, "list": [t.clone() for t in lst], "embedded": seen["ref"], "embed_false_returns_list": keep_is_returned,
            "invalid_raises": _raises(ns["preprocess_inputs"], C.preprocess_stand_in("x", {}), [3.14])}


def image_prefix_pins(ref):
    """ImagePrefix.forward (image_prefix.py:78-109, with the file's own ENCODER_SEQ_LENS table and einops.rearrange) on a stand-in
    `self` whose encoder / Linear / LayerNorm carry the oracle's tensors: the output, and the encoder features it was handed;
    the pooled-encoder branch on given features."""
    import torch.nn as nn
    from einops import rearrange
    import oracle.model as om
    path = os.path.join(ref, "magma/image_prefix.py")
    ns = {"torch": torch, "nn": nn, "rearrange": rearrange, "TensorType": sys.modules["torchtyping"].TensorType}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("ENCODER_SEQ_LENS", "ENCODER_OUT_DIMS"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    _methods(ref, "magma/image_prefix.py", "ImagePrefix", ("forward",), ns)
    cfg, p, images, (Cf, S, d, pp, feats) = C.image_prefix_inputs()

    def linear(w, b):
        m = nn.Linear(w.shape[1], w.shape[0])
        m.weight.data, m.bias.data = w.clone(), b.clone()
        return m
    ln = nn.LayerNorm(cfg.d_model, eps=cfg.ln_eps)
    ln.weight.data, ln.bias.data = p["image_prefix.ln.weight"].clone(), p["image_prefix.ln.bias"].clone()
    enc = {}

    def encoder(x):
        enc["in"], enc["out"] = x.clone(), om.encoder_fwd(p, cfg, x)
        return enc["out"].clone()
    fake = types.SimpleNamespace(enc=encoder, encoder_type="clip_resnet_large", dropout=nn.Identity(),
                                 proj=linear(p["image_prefix.proj.weight"], p["image_prefix.proj.bias"]), use_layernorm=cfg.use_prefix_ln,
                                 ln=ln, out_dim=cfg.d_model, out_seq_len=None)
    ln2 = nn.LayerNorm(d)
    ln2.weight.data, ln2.bias.data = pp["image_prefix.ln.weight"].clone(), pp["image_prefix.ln.bias"].clone()
    fake2 = types.SimpleNamespace(enc=lambda x: feats[:, :, None, None], encoder_type="nfresnet50", dropout=nn.Identity(),
                                  proj=linear(pp["image_prefix.proj.weight"], pp["image_prefix.proj.bias"]), use_layernorm=True, ln=ln2,
                                  out_dim=d, out_seq_len=S)
    with torch.no_grad():
        got, got2 = ns["forward"](fake, images), ns["forward"](fake2, images)
    return {"seq_len_clip_resnet_large": ns["ENCODER_SEQ_LENS"]["clip_resnet_large"], "sequence": got.clone(),
            "encoder_got_images": torch.equal(enc["in"], images), "encoder_out": enc["out"], "pooled": got2.clone()}


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "magma")):
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    _shim_torchtyping()
    pins = {"config": config_pins(ref), "dataset": dataset_pins(ref), "param_groups": param_group_pins(ref),
            "steps": step_pins(ref), "checkpoint": checkpoint_pins(ref),
            "plumbing": plumbing_pins(ref), "add_adapters": add_adapters_pins(ref), "preprocess_inputs": preprocess_inputs_pins(ref),
            "image_prefix": image_prefix_pins(ref)}
    torch.save(pins, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
