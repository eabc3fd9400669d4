"""CPU-side checks: config loading, C-ABI symbol export, loud failure without a
GPU, encoder bookkeeping, label oracle edge cases, synthetic data contract."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_cases as RC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# what the reference's own host-side code returned on the inputs of tests/reference_cases.py, run in place by
# tests/golden/make_host_golden.py; the published YAMLs it ran on are kept next to it in golden/reference_configs/
REF_PINS = torch.load(os.path.join(GOLDEN, "reference_host_pins.pt"), weights_only=False)
REF_CONFIGS = os.path.join(GOLDEN, "reference_configs")


def test_configs_parse_like_the_reference():
    from magma_amd.config import MultimodalConfig
    v1 = MultimodalConfig.from_yml("MAGMA_v1")
    assert v1.encoder_name == "clip_resnet_large" and v1.adapter_config["mlp"]["downsample_factor"] == 4
    assert v1.lr == 8e-4 and v1.image_enc_lr == 2e-6 and v1.gradient_accumulation_steps == 8
    assert v1.lr_scheduler == "WarmupDecayLR" and v1.deepspeed_config_params["scheduler"]["params"]["total_num_steps"] == 300000
    v2 = MultimodalConfig.from_yml(os.path.join(ROOT, "configs", "MAGMA_v2.yml"))
    assert set(v2.adapter_config) == {"mlp", "attention"} and v2.adapter_config["attention"]["downsample_factor"] == 8
    assert v2.extra.get("dataset_type") == "new"          # unknown keys are kept, not fatal
    # the published YAMLs (kept as data in tests/golden/reference_configs/) parse unchanged
    r1 = MultimodalConfig.from_yml(os.path.join(REF_CONFIGS, "MAGMA_v1.yml"))
    r2 = MultimodalConfig.from_yml(os.path.join(REF_CONFIGS, "MAGMA_v2.yml"))
    for f in RC.CONFIG_FIELDS:
        assert getattr(r1, f) == getattr(v1, f), f
        assert getattr(r2, f) == getattr(v2, f), f
    assert set(r2.extra) == set(RC.V2_EXTRA_KEYS)


def test_reduced_config_helper_adapter_sets():
    """magma_amd.testing.tiny_multimodal_config: the adapter sets the tests build (reference magma.py:111-120 adds each adapter
    only when adapter_config names it)."""
    from magma_amd.testing import tiny_multimodal_config as tiny
    assert tiny().adapter_config == {"mlp": {"adapter_type": "normal", "downsample_factor": 4}}
    assert set(tiny(8, 8).adapter_config) == {"mlp", "attention"}
    assert tiny(mlp_factor=None).adapter_config == {}
    assert tiny(mlp_factor=None, attn_factor=8, attn_type="scaled_parallel").adapter_config == {
        "attention": {"adapter_type": "scaled_parallel", "downsample_factor": 8}}
    assert not tiny(adapter_config=None).adapter_config
    assert tiny(mlp_factor=None, adapter_config={"attention": {"adapter_type": "parallel"}}).adapter_config == {
        "attention": {"adapter_type": "parallel"}}


def test_library_exports_every_declared_symbol():
    """include/magma_hip.h is the contract: every function it declares must be
    exported by the built library and bound by magma_amd.lib (no compute calls here)."""
    from magma_amd import lib
    header = open(os.path.join(ROOT, "include", "magma_hip.h")).read()
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", header))
    declared -= {"mg_epilogue", "mg_gemm_desc", "mg_skinny_desc"}
    assert declared == set(lib.SYMBOLS), declared ^ set(lib.SYMBOLS)
    if not lib.LIB_PATH.exists():
        pytest.skip("libmagma_hip.so not built (run __graft_entry__.build())")
    try:
        dll = ctypes.CDLL(str(lib.LIB_PATH))
    except OSError as e:
        pytest.skip(f"cannot dlopen the HIP library here: {e}")
    for name in declared:
        assert hasattr(dll, name), f"{name} declared in the header but not exported"


def test_no_cpu_fallback():
    from magma_amd import Magma, ops
    from magma_amd.lib import MagmaHipError
    with pytest.raises(MagmaHipError):
        Magma("MAGMA_v1", device="cpu")
    with pytest.raises(MagmaHipError):
        ops.layernorm(torch.zeros(2, 64, dtype=torch.bfloat16), torch.ones(64), torch.zeros(64))
    import magma_amd
    src = "".join(open(os.path.join(ROOT, "magma_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "magma_amd"))
                  if f.endswith(".py"))
    assert "import oracle" not in src and "from oracle" not in src, "product code must not import the oracle"


def test_encoder_spec_matches_reference_constants():
    from oracle.model import OracleConfig, enc_conv_specs
    cfg = OracleConfig.magma_v1()
    specs = enc_conv_specs(cfg)
    assert len(specs) == 127 and sum(1 for s in specs if s[3] == 3) == 43
    n_params = sum(ci * co * k * k + 2 * co for _, ci, co, k in specs)
    assert abs(n_params / 1e6 - 136.2) < 0.05
    assert cfg.enc_out_dim == 3072                                  # reference image_prefix.py:20
    from magma_amd.image_prefix import ENCODER_OUT_DIMS, ENCODER_SEQ_LENS
    assert ENCODER_OUT_DIMS["clip_resnet_large"] == 3072 and ENCODER_SEQ_LENS["clip_resnet_large"] == 144


def test_encoder_module_names_match_clip():
    from magma_amd.image_encoders import ModifiedResNetTrunk
    from oracle.model import OracleConfig, init_params
    cfg = OracleConfig.tiny()
    enc = ModifiedResNetTrunk(cfg.enc_layers, cfg.enc_width, 64)
    own = set(k for k in enc.state_dict() if not k.endswith("num_batches_tracked"))
    want = set(k[len("image_prefix.enc."):] for k in init_params(cfg, 0) if k.startswith("image_prefix.enc."))
    assert own == want


def test_oracle_encoder_shapes():
    from oracle.model import OracleConfig, encoder_fwd, init_params
    cfg = OracleConfig.tiny()
    p = init_params(cfg, 0)
    out = encoder_fwd(p, cfg, torch.randn(1, 3, 96, 64))
    assert out.shape == (1, 3 * 2, cfg.enc_out_dim)


def test_synthetic_data_contract():
    from magma_amd.datasets import synthetic_batch
    imgs, caps = synthetic_batch(3, 64, 128, eos=50256, vocab=50256, seed=1)
    assert imgs.shape == (3, 3, 64, 64) and caps.shape == (3, 128) and caps.dtype == torch.int64
    first = (caps == 50256).int().argmax(1)
    assert bool(((first >= 8) & (first <= 64)).all())
    for r, f in zip(caps, first):
        assert bool((r[f:] == 50256).all())


def test_tokenizer_contract():
    from magma_amd.tokenizer import get_tokenizer
    tok = get_tokenizer("gpt2", 2048)
    assert tok.eos_token_id == 50256 and tok.cls_token_id == 50257 and len(tok) == 50258
    ids = tok.encode("Describe the painting:", return_tensors="pt")
    assert ids.ndim == 2 and ids.dtype == torch.int64


def test_clip_preprocess_shape_and_stats():
    import PIL.Image as I
    import numpy as np
    from magma_amd.transforms import clip_preprocess
    img = I.fromarray((np.random.RandomState(0).rand(300, 224, 3) * 255).astype("uint8"))
    t = clip_preprocess(384)(img)
    assert t.shape == (1, 3, 384, 384) and t.dtype == torch.float32
    assert abs(float(t.mean())) < 0.5


def test_host_side_label_index_matches_build_labels():
    """MagmaEngine.target_index (the loss head's row / label plumbing, computed on the host so that the training step has no
    device sync) against the reference's label rule as the oracle states it (reference utils.py:334-364)."""
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import build_labels
    g = torch.Generator().manual_seed(0)
    for P in (0, 4, 49):
        S, eos = 96 + P, 7
        caps = torch.randint(8, 50, (6, S), generator=g)
        caps[0, :] = 9                    # no eos at all
        caps[1, 0] = eos                  # eos first
        caps[2, 5] = eos
        caps[3, S - P - 1] = eos          # eos in the last kept position
        caps[4, 3] = eos; caps[4, 10] = eos
        rows, tgt, first = MagmaEngine.target_index(caps, P, eos, S)
        lab = build_labels(P, caps, eos)
        t = lab[:, 1:].reshape(-1)
        allrows = (torch.arange(6)[:, None] * S + torch.arange(S - 1)[None, :]).reshape(-1)
        keep = (t != -100).nonzero().squeeze(1)
        assert torch.equal(rows, allrows[keep]) and torch.equal(tgt, t[keep]), P
        assert first.tolist()[:5] == [S - P - 1, 0, 5, S - P - 1, 3]


def test_lazy_loss_and_magma_alias():
    from magma_amd.train_loop import LazyLoss
    x = LazyLoss(torch.tensor(1.25))
    assert f"{x:.2f}" == "1.25" and float(x) == 1.25 and x.item() == 1.25 and x < 2 and x > 1 and str(x) == "1.25"
    import magma
    import magma_amd
    from magma.image_input import ImageInput
    assert magma.Magma is magma_amd.Magma and ImageInput is magma_amd.ImageInput
    from magma import collate_fn, eval_step, inference_step, train_step   # noqa: F401  (reference magma/__init__.py:19-20)


def test_img_cpt_dataset_reads_the_reference_layout(tmp_path):
    """reference magma/datasets/dataset.py:92-160: <dir>/image_data/<shard>/<n>.json records + images relative to <dir>;
    items (1,3,H,W) / (1,seq_len) right-padded with eos; collate -> (B,3,H,W), (B,seq_len)."""
    import json
    import numpy as np
    import PIL.Image as I
    from magma_amd.datasets import ImgCptDataset, collate_fn
    from magma_amd.tokenizer import ByteTokenizer
    from magma_amd.transforms import clip_preprocess
    (tmp_path / "image_data" / "00000").mkdir(parents=True)
    (tmp_path / "images" / "00000").mkdir(parents=True)
    rng = np.random.RandomState(0)
    for i in range(3):
        I.fromarray((rng.rand(50 + i, 70, 3) * 255).astype("uint8")).save(tmp_path / "images" / "00000" / f"{i}.jpg")
        rec = {"captions": [f"caption {i}"], "metadata": {}}
        if i != 1:
            rec["image_path"] = f"images/00000/{i}.jpg"          # record 1: path inferred from the record's own name
        (tmp_path / "image_data" / "00000" / f"{i}.json").write_text(json.dumps(rec))
    ds = ImgCptDataset(tmp_path, ByteTokenizer(64), clip_preprocess(32), seq_len=64)
    assert len(ds) == 3
    img, cap = ds[1]
    assert img.shape == (1, 3, 32, 32) and cap.shape == (1, 64) and cap.dtype == torch.int64
    assert cap[0, :9].tolist() == list(b"caption 1") and bool((cap[0, 9:] == ByteTokenizer.eos_token_id).all())
    images, caps = collate_fn([ds[i] for i in range(3)], seq_len=64)
    assert images.shape == (3, 3, 32, 32) and caps.shape == (3, 64)


def test_loader_workers_iterate_a_host_side_view(tmp_path):
    """train_engine.deepspeed_io with worker processes (reference train.py:103-112: DeepSpeed's loader runs workers): the
    workers iterate datasets.host_side_view -- every ImgCptDataset under Subset / ConcatDataset wrappers with its transform
    replaced by the host-only twin (same pixels, CPU tensors) -- and a real DataLoader with 2 worker processes + the
    default collate yields the batches of the in-process loader."""
    from functools import partial
    from magma_amd.datasets import ImgCptDataset, collate_fn, host_side_view, on_disk, SyntheticImgCptDataset
    from magma_amd.tokenizer import ByteTokenizer
    from magma_amd.transforms import clip_preprocess
    _write_dataset(tmp_path, 6, modes=("RGB", "L"))
    calls = []
    host = clip_preprocess(32)
    assert host.host is host                          # a host transform is its own host-side twin

    def device_like(img):                             # stands in for the device pipeline: must never run in a worker
        calls.append(1)
        return host(img)
    device_like.host = host
    ds = ImgCptDataset(tmp_path, ByteTokenizer(64), device_like, seq_len=64)
    sub = torch.utils.data.Subset(ds, [4, 2, 0, 1])
    cat = torch.utils.data.ConcatDataset([sub, ds])
    view = host_side_view(cat)
    assert on_disk(cat) and not on_disk(SyntheticImgCptDataset(4, 32, 64))
    assert isinstance(view, torch.utils.data.ConcatDataset) and isinstance(view.datasets[0], torch.utils.data.Subset)
    assert view.datasets[0].indices == [4, 2, 0, 1] and view.datasets[0].dataset.transforms is host and view.datasets[1].transforms is host
    assert ds.transforms is device_like               # the original keeps its transform
    assert host_side_view(SyntheticImgCptDataset(4, 32, 64)).__class__ is SyntheticImgCptDataset
    ref = [b for b in torch.utils.data.DataLoader(host_side_view(sub), batch_size=2, collate_fn=partial(collate_fn, seq_len=64))]
    assert not calls
    got = [b for b in torch.utils.data.DataLoader(host_side_view(sub), batch_size=2, num_workers=2,
                                                  collate_fn=partial(collate_fn, seq_len=64))]
    assert len(got) == len(ref) == 2
    for (gi, gc), (ri, rc) in zip(got, ref):
        assert gi.shape == (2, 3, 32, 32) and torch.equal(gi, ri) and torch.equal(gc, rc)
    # the engine's loader SPAWNS its workers (train_engine.deepspeed_io: no fork of a process that holds HIP / RCCL state): the
    # dataset view, its transform (a picklable class since round 6) and the collate function travel by pickle
    real = torch.utils.data.Subset(ImgCptDataset(tmp_path, ByteTokenizer(64), clip_preprocess(32), seq_len=64), [4, 2, 0, 1])
    spawned = [b for b in torch.utils.data.DataLoader(host_side_view(real), batch_size=2, num_workers=2, multiprocessing_context="spawn",
                                                      collate_fn=partial(collate_fn, seq_len=64))]
    for (gi, gc), (ri, rc) in zip(spawned, ref):
        assert torch.equal(gi, ri) and torch.equal(gc, rc)


def _write_dataset(root, n, modes=("RGB",)):
    import json
    import numpy as np
    import PIL.Image as I
    (root / "image_data" / "00000").mkdir(parents=True)
    (root / "images" / "00000").mkdir(parents=True)
    rng = np.random.RandomState(0)
    for i in range(n):
        mode = modes[i % len(modes)]
        arr = (rng.rand(40 + i, 56) * 255).astype("uint8") if mode == "L" else (rng.rand(40 + i, 56, 3) * 255).astype("uint8")
        I.fromarray(arr).save(root / "images" / "00000" / f"{i}.png")
        rec = {"captions": [f"caption {i}"], "image_path": f"images/00000/{i}.png"}
        (root / "image_data" / "00000" / f"{i}.json").write_text(json.dumps(rec))


def test_mixed_mode_images_collate(tmp_path):
    """A greyscale image next to an RGB one (common in COCO / CC3M) through the dataset + collate_fn: both branches of
    the transform must land on one device and in one shape (reference transforms.py:121-134 converts AFTER the resize)."""
    from magma_amd.datasets import ImgCptDataset, collate_fn
    from magma_amd.tokenizer import ByteTokenizer
    from magma_amd.transforms import clip_preprocess
    _write_dataset(tmp_path, 4, modes=("RGB", "L"))
    ds = ImgCptDataset(tmp_path, ByteTokenizer(32), clip_preprocess(24), seq_len=32)
    items = [ds[i] for i in range(4)]
    assert len({it[0].device for it in items}) == 1
    images, caps = collate_fn(items, seq_len=32)
    assert images.shape == (4, 3, 24, 24) and caps.shape == (4, 32)
    grey = items[1][0]          # a grey image: the three normalised channels are the same pixel values
    from magma_amd.transforms import CLIP_MEAN, CLIP_STD
    back = [grey[0, c] * CLIP_STD[c] + CLIP_MEAN[c] for c in range(3)]
    assert torch.allclose(back[0], back[1], atol=1e-6) and torch.allclose(back[1], back[2], atol=1e-6)


def test_pretraining_datasets_follow_the_reference_rules(tmp_path):
    """reference train.py:34-66: list -> ConcatDataset, eval_dataset_dir None -> eval_dataset_pct split of the train set,
    wrong type -> TypeError; a missing directory raises instead of silently training on noise; only the literal
    'synthetic' selects synthetic data."""
    from types import SimpleNamespace
    from magma_amd.datasets import SyntheticImgCptDataset, get_pretraining_datasets, load_img_cpt_datasets
    from magma_amd.tokenizer import ByteTokenizer
    from magma_amd.transforms import clip_preprocess
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    _write_dataset(a, 6)
    _write_dataset(b, 4)
    tok, tf = ByteTokenizer(32), clip_preprocess(16)
    cfg = SimpleNamespace(train_dataset_dir=[str(a), str(b)], eval_dataset_dir=None, eval_dataset_pct=0.2)
    train, evals = get_pretraining_datasets(cfg, tok, tf, seq_len=32, split_seed=0)
    assert len(train) == 8 and len(evals) == 2
    t2, e2 = get_pretraining_datasets(cfg, tok, tf, seq_len=32, split_seed=0)
    assert list(evals.indices) == list(e2.indices)                         # same split on every rank
    assert isinstance(train.dataset, torch.utils.data.ConcatDataset)
    assert train[0][0].shape == (1, 3, 16, 16)
    cfg = SimpleNamespace(train_dataset_dir=str(a), eval_dataset_dir=str(b), eval_dataset_pct=0.1)
    train, evals = get_pretraining_datasets(cfg, tok, tf, seq_len=32)
    assert len(train) == 6 and len(evals) == 4
    with pytest.raises(FileNotFoundError):
        load_img_cpt_datasets(str(tmp_path / "typo"), tok, tf)
    with pytest.raises(TypeError):
        load_img_cpt_datasets(3, tok, tf)
    with pytest.raises(ValueError):
        load_img_cpt_datasets("synthetic", tok, tf)
    syn = load_img_cpt_datasets("synthetic", tok, tf, synthetic=lambda: SyntheticImgCptDataset(5, 16, 32))
    assert len(syn) == 5
    cfg = SimpleNamespace(train_dataset_dir="synthetic", eval_dataset_dir=None, eval_dataset_pct=0.1)
    train, evals = get_pretraining_datasets(cfg, tok, tf, 32, synthetic_train=lambda: SyntheticImgCptDataset(50, 16, 32))
    assert len(train) == 45 and len(evals) == 5


def test_nfresnet50_structure_matches_timm_constants():
    """nf_resnet50 as the reference wraps it (image_encoders.py:31-45): 53 scaled-std convs, 25,557,032 parameters with timm's
    2048 -> 1000 classifier (the published count of timm nf_resnet50), 2048 output channels (image_prefix.py:17); the
    product module's state-dict keys are exactly the oracle's, i.e. the reference's ``0.0.conv.*`` / ``0.1.{s}.{b}.*`` names."""
    from magma_amd.image_encoders import NFResNet50
    from oracle.nfnet import NFResNetConfig, block_plan, conv_specs, encoder_fwd, init_params
    c = NFResNetConfig()
    specs = conv_specs(c)
    assert len(specs) == 53
    assert sum(cin * cout * k * k + 2 * cout for _, cin, cout, k in specs) + 2048 * 1000 + 1000 == 25_557_032
    p = init_params(c, seed=0, prefix="")
    enc = NFResNet50(256)
    assert set(enc.state_dict().keys()) == set(p.keys())
    assert all(enc.state_dict()[k].shape == p[k].shape for k in p)
    betas = [round(b, 4) for _, _, _, b in block_plan(c)]
    assert betas[:4] == [1.0, 0.9806, 0.9623, 0.9449] and betas[7] == 0.9285      # stage boundaries keep the running variance
    for (_, _, _, b), blk in zip(block_plan(c), [blk for st in enc.stages for blk in st]):
        assert abs(b - blk.beta) < 1e-12
    y = encoder_fwd(init_params(c, seed=1), c, torch.randn(1, 3, 64, 64))
    assert y.shape == (1, 2048) and bool((y >= 0).all())


def test_base_transforms_contract():
    """reference transforms.py:65-84 (non-CLIP encoders): any mode / size -> (1, 3, image_size, image_size) in [0, 1]."""
    import numpy as np
    import PIL.Image as I
    from magma_amd.transforms import get_transforms, pad_to_size
    tf = get_transforms(128, "nfresnet50")
    rng = np.random.default_rng(0)
    for shape, mode in [((200, 300, 3), "RGB"), ((90, 70), "L"), ((400, 130, 3), "RGB")]:
        img = I.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), mode=mode)
        t = tf(img)
        assert t.shape == (1, 3, 128, 128) and t.dtype == torch.float32 and 0.0 <= float(t.min()) and float(t.max()) <= 1.0
    assert pad_to_size(I.new("RGB", (100, 60)), 128).size == (128, 128)
    torch.manual_seed(0); import random; random.seed(0)
    a = tf(I.fromarray(rng.integers(0, 256, (150, 150, 3), dtype=np.uint8)))
    assert a.shape == (1, 3, 128, 128)


def test_workspace_query_is_consistent_with_the_split_policy():
    """mg_gemm_workspace_bytes (callers own all memory): 0 for shapes that fill the chip, else splits x M x
    ceil(N/128)*128 fp32 (or the larger need of the split 256x256 form) -- pure host arithmetic, callable without a GPU."""
    import ctypes
    from magma_amd import lib
    if not lib.LIB_PATH.exists():
        pytest.skip("libmagma_hip.so not built")
    try:
        dll = ctypes.CDLL(str(lib.LIB_PATH))
    except OSError as e:
        pytest.skip(f"cannot dlopen the HIP library here: {e}")
    f = dll.mg_gemm_workspace_bytes
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int32] * 3
    assert f(32768, 16384, 4096) == 0                       # training shape: 32768 tiles
    assert f(456, 4096, 16384) == 8 * 456 * 4096 * 4        # prefill fc_out: 2 x 16 tiles of 256x256 -> 8-way split (the 128x128 form: 4-way)
    assert f(4096, 1024, 32768) == 4 * 4096 * 1024 * 4      # adapter weight gradient: 16 x 4 tiles of 256x256 -> 4-way split
    assert f(456, 1024, 4096) == 16 * 456 * 1024 * 4        # adapter-down: 32 tiles -> 16-way
    assert f(0, 1, 1) == 0


def test_config_equals_the_reference_class_run_in_place():
    """reference magma/config.py:20-144 (MultimodalConfig + the derived DeepSpeed dictionary: optimizer, WarmupDecayLR parameters, ZeRO
    stage, clipping, micro-batch arithmetic), run in place on the published YAMLs (tests/golden/make_host_golden.py): every dataclass
    field and the whole derived dictionary equal this repo's MultimodalConfig on the same files.  The reference class REJECTS its own
    MAGMA_v2.yml (three keys that are not fields) -- pinned as well; with those keys dropped the two classes agree on v2 too."""
    from magma_amd.config import MultimodalConfig
    pins = REF_PINS["config"]
    m1 = MultimodalConfig.from_yml(os.path.join(REF_CONFIGS, "MAGMA_v1.yml"))
    assert len(pins["v1"]) >= 40
    for k, v in pins["v1"].items():
        if k == "name":                       # a random uuid4 prefix on both sides when the YAML gives none (reference config.py)
            assert isinstance(m1.name, str) and len(m1.name) == len(v)
            continue
        assert getattr(m1, k) == v, k
    assert pins["v1_deepspeed"] == m1.deepspeed_config_params
    assert pins["v2_from_yml_raises"] == "TypeError"
    m2 = MultimodalConfig.from_yml(os.path.join(REF_CONFIGS, "MAGMA_v2.yml"))
    for k, v in pins["v2"].items():
        assert k == "name" or getattr(m2, k) == v, k
    assert pins["v2_deepspeed"] == m2.deepspeed_config_params and m2.extra == pins["v2_extra"]
    assert set(pins["v2_extra"]) == set(RC.V2_EXTRA_KEYS)


def test_dataset_equals_the_reference_class_run_in_place(tmp_path):
    """reference magma/datasets/dataset.py:92-160 (ImgCptDataset over the LazyLoader, collate_fn), run in place by
    tests/golden/make_host_golden.py on an on-disk dataset in the reference's layout -- two shards, a record without image_path (path
    inferred from the record's name), greyscale and RGB images -- with the same tokenizer and transform objects as this repo's reader:
    same length, same order, identical tensors per item, identical batches from collate_fn (single-caption records: the reference
    draws the caption with random.choice)."""
    from magma_amd.datasets import ImgCptDataset, collate_fn
    pins = REF_PINS["dataset"]
    RC.write_dataset(tmp_path)
    tok, tf = RC.dataset_tokenizer_and_transform()
    mine = ImgCptDataset(tmp_path, tok, tf, seq_len=RC.DATASET_SEQ_LEN)
    assert len(pins["items"]) == len(mine) == 8
    items_m = [mine[i] for i in range(8)]
    for (it, ct), (im, cm) in zip(pins["items"], items_m):
        assert it.shape == im.shape and torch.equal(it, im)
        assert ct.dtype == cm.dtype and torch.equal(ct, cm)
    bt, bm = pins["collate"], collate_fn(items_m, seq_len=RC.COLLATE_SEQ_LEN)
    assert torch.equal(bt[0], bm[0]) and torch.equal(bt[1], bm[1]) and bm[1].shape == (8, RC.COLLATE_SEQ_LEN)


@pytest.mark.parametrize("weight_decay,image_enc_lr,use_ln", [(0.0, 2e-6, True), (0.05, 2e-6, True), (0.05, None, False), (0.0, 2e-6, False)])
def test_param_groups_equal_the_reference_functions_run_in_place(weight_decay, image_enc_lr, use_ln):
    """reference magma/utils.py:120-238 (get_params_for_weight_decay_optimization + configure_param_groups; utils.py itself needs
    deepspeed / wandb / gdown, so tests/golden/make_host_golden.py extracts the two FunctionDefs with ast and runs them in place) on a
    model with the reference's attribute structure (image_prefix.enc / .proj / .ln, lm with Embedding / LayerNorm / Linear + frozen
    tensors): the same groups in the same order -- per group the same (lr, weight_decay) and the same parameters in the same order --
    and the same warmup_min_lr / warmup_max_lr lists written into the scheduler parameters."""
    from magma_amd.utils import configure_param_groups
    pins = REF_PINS["param_groups"][(weight_decay, image_enc_lr, use_ln)]
    model = RC.param_group_model(use_ln)
    cfg = RC.param_group_config(weight_decay, image_enc_lr, use_ln)
    mine = configure_param_groups(model, cfg)
    assert all(isinstance(p, torch.nn.Parameter) for g in mine for p in g["params"])
    assert RC.describe_param_groups(model, mine) == pins["groups"]
    assert cfg.deepspeed_config_params == pins["deepspeed"]


@pytest.mark.parametrize("run_blind", [False, True])
def test_train_and_eval_step_equal_the_reference_functions_run_in_place(run_blind):
    """reference magma/train_loop.py:7-21,48-60 (train_step / eval_step) and utils.py:26-34 (reduce_losses), run in place by
    tests/golden/make_host_golden.py against a recording engine; this repo's train_loop on the same engine and the same loader: the
    same sequence of engine calls (gradient_accumulation_steps x {forward, backward, step}; eval_steps x forward), the same captions,
    images zeroed under run_blind, the same returned mean loss.  (The reference moves its batch with .half().cuda(), kept on the host
    for the pins; this repo's loop moves it to engine.device in bf16 -- the dtype is the documented difference.)"""
    from magma_amd import train_loop as mine
    for fn_mine, name, n_calls in ((mine.train_step, "train_step", 3), (mine.eval_step, "eval_step", 2)):
        pin = REF_PINS["steps"][(run_blind, name)]
        e_mine = RC.RecordingEngine()
        l_mine = fn_mine(RC.step_config(run_blind), RC.step_loader(), e_mine)
        assert float(l_mine) == pytest.approx(pin["loss"]) == pytest.approx(sum(0.5 * (i + 1) for i in range(n_calls)) / n_calls)
        assert [ev[0] for ev in pin["events"]] == [ev[0] for ev in e_mine.events]
        for a, b in zip(pin["events"], e_mine.events):
            if a[0] == "forward":
                assert a[1] == b[1] and a[2] == b[2] == run_blind and torch.equal(a[3], b[3])
            else:
                assert a == b


def test_checkpoint_helpers_equal_the_reference_functions_run_in_place(tmp_path):
    """reference magma/utils.py:89-117 (save_model / load_model) and :285-308 (infer_checkpoint_path_from_config), extracted with ast and
    run in place by tests/golden/make_host_golden.py; this repo's functions on the same recording engine and the same directory trees:
    the same client state and config.yml written, the same resume step returned (0 when the engine reports a failed load), the same
    path found through the `latest` tag and the same ValueErrors for a missing folder / tag / file."""
    from magma_amd import utils as mine
    got = RC.checkpoint_helpers_run(mine.save_model, mine.load_model, mine.infer_checkpoint_path_from_config, tmp_path)
    pin = REF_PINS["checkpoint"]
    assert pin["load"] == [1234, 0, 1234] and pin["save_none"] == "ValueError"
    assert [r[0] for r in pin["infer"]] == ["ValueError", "ValueError", "ok"]
    assert got == pin


def test_from_checkpoint_signature_and_safe_unpickle(tmp_path, monkeypatch):
    """reference magma.py:278-279: from_checkpoint(config_path, checkpoint_path, device='cpu') -- the signature is kept, and since
    there is no CPU execution path the default fails loudly NAMING the fix.  The file itself is read with the safe unpickler
    (DeepSpeed's Namespace / numpy scalars allow-listed); a payload that needs code execution is refused unless
    MAGMA_UNSAFE_UNPICKLE=1."""
    import argparse
    import inspect
    import numpy as np
    from magma_amd import Magma
    from magma_amd.lib import MagmaHipError
    from magma_amd.magma import _load_checkpoint_file
    sig = inspect.signature(Magma.from_checkpoint)
    assert list(sig.parameters)[:3] == ["config_path", "checkpoint_path", "device"] and sig.parameters["device"].default == "cpu"
    path = tmp_path / "mp_rank_00_model_states.pt"
    torch.save({"module": {"w": torch.ones(2)}, "global_steps": 3, "args": argparse.Namespace(lr=8e-4), "skipped_steps": np.int64(0),
                "scale": np.float32(2.5), "ds_version": "0.3.15"}, path)
    with pytest.raises(MagmaHipError, match="device='cuda:0'"):
        Magma.from_checkpoint("MAGMA_v1", str(path))
    sd = _load_checkpoint_file(str(path))
    assert sd["args"].lr == 8e-4 and int(sd["skipped_steps"]) == 0 and torch.equal(sd["module"]["w"], torch.ones(2))

    class Payload:
        def __reduce__(self):
            return (exec, ("import os; os.environ['MAGMA_TEST_PAYLOAD_RAN'] = '1'",))

    torch.save({"module": {"w": torch.ones(2)}, "x": Payload()}, path)
    monkeypatch.delenv("MAGMA_UNSAFE_UNPICKLE", raising=False)
    monkeypatch.delenv("MAGMA_TEST_PAYLOAD_RAN", raising=False)
    with pytest.raises(RuntimeError, match="MAGMA_UNSAFE_UNPICKLE"):
        _load_checkpoint_file(str(path))
    assert "MAGMA_TEST_PAYLOAD_RAN" not in os.environ
    monkeypatch.setenv("MAGMA_UNSAFE_UNPICKLE", "1")
    with pytest.warns(RuntimeWarning, match="full unpickle"):
        assert "module" in _load_checkpoint_file(str(path))
    assert os.environ.pop("MAGMA_TEST_PAYLOAD_RAN", None) == "1"


def test_lm_output_lazy_values_resolve_on_every_conversion():
    """dict(out), {**out}, out.copy() and pickling must not hand out the raw lazy closure; is_lazy() asks
    without computing."""
    import pickle
    from magma_amd.language_model import LMOutput
    calls = []

    def make():
        return LMOutput(loss=torch.tensor(1.0), logits=LMOutput.lazy(lambda: (calls.append(1), torch.ones(2))[1]))

    o = make()
    assert o.is_lazy("logits") and not o.is_lazy("loss") and not calls
    assert isinstance(dict(make())["logits"], torch.Tensor)
    assert isinstance({**make()}["logits"], torch.Tensor)
    assert isinstance(make().copy()["logits"], torch.Tensor)
    back = pickle.loads(pickle.dumps(make()))
    assert isinstance(back, LMOutput) and torch.equal(back.logits, torch.ones(2))
    n = len(calls)
    assert o.logits is o.logits and len(calls) == n + 1 and not o.is_lazy("logits")      # computed once, then stored


def test_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """The descriptors cross the C ABI by value-in-memory: every ctypes mirror in magma_amd/lib.py (and with it the stub in
    INTEGRATION.md) must have the size and the field offsets the C compiler gives include/magma_hip.h.  gcc compiles a probe
    that prints offsetof() of every field; compared field by field."""
    import ctypes as C
    import subprocess
    from magma_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"mg_epilogue": L.Epilogue, "mg_gemm_desc": L.GemmDesc, "mg_skinny_desc": L.SkinnyDesc,
               "mg_relayout_job": L.RelayoutJob, "mg_bn_fold_job": L.BnFoldJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "magma_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("abi %d\\n", MG_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        parts = ln.split()
        got[tuple(parts[:-1])] = int(parts[-1])
    assert got[("abi",)] == L.ABI_VERSION
    for cname, cls in structs.items():
        assert got[(cname, "size")] == C.sizeof(cls), (cname, got[(cname, "size")], C.sizeof(cls))
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    # the stub in INTEGRATION.md names the same epilogue fields in the same order
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    stub = text[text.index("class mg_epilogue(C.Structure)"):text.index("class mg_gemm_desc(C.Structure)")]
    import re
    assert re.findall(r'\("(\w+)",', stub) == [f for f, _ in L.Epilogue._fields_]


def test_labels_outside_the_head_vocabulary_are_refused_on_the_host():
    """A caption id >= V (a tokenizer wider than the head) reaches the loss head through MagmaEngine.target_index unchanged; the
    kernels would ignore such a target and the embedding gather clamps the id, so the engines refuse it where the labels are on
    the host: ValueError naming the id and V."""
    from magma_amd import ops
    from magma_amd.train_engine import MagmaEngine
    V, eos, P = 50, 7, 4
    S = 24 + P
    caps = torch.randint(8, V, (3, S), generator=torch.Generator().manual_seed(1))
    caps[:, 20] = eos
    rows, tgt, _ = MagmaEngine.target_index(caps, P, eos, S)
    assert int(tgt.max()) < V and int(tgt.min()) >= 0 and tgt.numel() == 3 * 21
    ops.refuse_targets_outside(tgt, V)                       # in range: silent
    ops.refuse_targets_outside(tgt[:0], V)                   # nothing to check
    caps[1, 5] = V                                           # the first id past the head
    rows, tgt, _ = MagmaEngine.target_index(caps, P, eos, S)
    assert int(tgt.max()) == V                               # target_index passes it on as it is
    with pytest.raises(ValueError, match=rf"\b{V}\b.*V = {V}\b"):
        ops.refuse_targets_outside(tgt, V)
    caps[1, 5] = 10 ** 6
    with pytest.raises(ValueError, match=rf"1000000.*V = {V}\b"):
        ops.refuse_targets_outside(MagmaEngine.target_index(caps, P, eos, S)[1], V)
    caps[1, 5] = -3
    with pytest.raises(ValueError, match=rf"-3.*V = {V}\b"):
        ops.refuse_targets_outside(MagmaEngine.target_index(caps, P, eos, S)[1], V)
    caps[1, 21] = 10 ** 6                                    # behind the first eos: masked, never a label
    caps[1, 5] = 9
    ops.refuse_targets_outside(MagmaEngine.target_index(caps, P, eos, S)[1], V)
