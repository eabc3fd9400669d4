"""encoder_name "nfresnet50" (reference magma/image_encoders.py:31-45, magma/image_prefix.py:17,67-72,96-101): timm's
NF-ResNet-50 + the pooled ImagePrefix branch on the HIP kernels against the oracle restatement (oracle/nfnet.py; timm is
un-vendored and absent: parity unpinned, see its header).  Tolerance: 2 x eager-bf16 + floor, as the other encoders."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def bf16_params(p):
    return {k: (v.to(BF16) if v.is_floating_point() else v) for k, v in p.items()}


def test_weight_standardize_kernel(dev):
    """mg_weight_standardize_bf16 against the oracle's statement of timm ScaledStdConv2d, both column orders."""
    from magma_amd import ops
    from oracle.nfnet import RELU_GAMMA, standardized_weight
    g = torch.Generator().manual_seed(0)
    for cout, cin, k in [(64, 3, 7), (64, 256, 1), (128, 128, 3), (40, 24, 3)]:
        w = (torch.randn(cout, cin, k, k, generator=g) + 0.5).to(BF16)
        gain = (1 + 0.2 * torch.randn(cout, 1, 1, 1, generator=g)).to(BF16)
        ref = standardized_weight(w.float(), gain.float(), 1e-5).reshape(cout, -1)
        fan_in = cin * k * k
        got = ops.weight_standardize(w.cuda(), gain.cuda().reshape(-1), RELU_GAMMA * fan_in ** -0.5, 1e-5, ldo=(fan_in + 15) // 8 * 8)
        assert bool((got[:, fan_in:] == 0).all())
        assert rel(got[:, :fan_in], ref) < 4e-3                 # bf16 rounding of the output only
        if k == 3:
            got2 = ops.weight_standardize(w.cuda(), gain.cuda().reshape(-1), RELU_GAMMA * fan_in ** -0.5, 1e-5, to_khwc=True)
            ref2 = standardized_weight(w.float(), gain.float(), 1e-5).permute(0, 2, 3, 1).reshape(cout, -1)
            assert rel(got2[:, :fan_in], ref2) < 4e-3


def test_pool_and_im2col_kernels(dev):
    from magma_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 16, 10, 14, generator=g).to(BF16)                   # NCHW reference tensors, NHWC for the kernels
    nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()
    mp = ops.maxpool3x3s2(nhwc).permute(0, 3, 1, 2).float().cpu()
    assert torch.equal(mp, F.max_pool2d(x.float(), 3, stride=2, padding=1))
    ss = ops.subsample2(nhwc).permute(0, 3, 1, 2).cpu()
    assert torch.equal(ss, x[:, :, ::2, ::2])
    rm = ops.relu_mean_rows(nhwc.view(2, 140, 16)).float().cpu()
    assert rel(rm, F.relu(x.float()).mean(dim=(2, 3))) < 4e-3
    img = torch.randn(2, 3, 18, 22, generator=g).to(BF16)
    cols = ops.im2col_nchw(img.cuda(), 7, 2, 3, 160).float().cpu()
    ref = F.unfold(img.float(), 7, padding=3, stride=2).transpose(1, 2).reshape(-1, 147)    # column (c, ky, kx)
    assert torch.equal(cols[:, :147], ref) and bool((cols[:, 147:] == 0).all())


@pytest.mark.parametrize("res", [96, 128, 224, 256])      # 96, 224: multiples of 32 that are not multiples of 64 (odd final map)
def test_nfresnet50_encoder_and_pooled_prefix(dev, res):
    """The full architecture (53 scaled-std convs, 23.5 M parameters) at two resolutions, then the pooled prefix on top."""
    from magma_amd.image_encoders import NFResNet50
    from magma_amd.image_prefix import ImagePrefix
    from magma_amd.testing import tiny_multimodal_config
    from oracle.model import pooled_prefix_fwd
    from oracle.nfnet import NFResNetConfig, encoder_fwd, init_params
    c = NFResNetConfig()
    p = init_params(c, seed=3)
    enc = NFResNet50(res, device=dev, dtype=BF16)
    enc.load_state_dict({k[len("image_prefix.enc."):]: t for k, t in p.items()}, strict=True)
    enc.invalidate_packed()
    x = torch.randn(2, 3, res, res, generator=torch.Generator().manual_seed(0)).to(BF16).float()
    with torch.no_grad():
        ref = encoder_fwd(p, c, x)
        eb = rel(encoder_fwd(bf16_params(p), c, x.to(BF16)), ref)
        got = enc(x.cuda())
    print(f"nf_resnet50 @{res}: HIP {rel(got, ref):.3e}, eager bf16 {eb:.3e}")
    assert got.shape == ref.shape == (2, 2048)
    assert rel(got, ref) <= 2 * eb + 5e-3, (rel(got, ref), eb)
    d, s = 512, 2
    cfg = tiny_multimodal_config(encoder_name="nfresnet50", image_seq_len=s, image_size=res)
    ip = ImagePrefix(cfg, out_dim=d, device=dev, dtype=BF16, enc=enc)
    assert ip.pooled and ip.out_seq_len == s and ip.proj.weight.shape == (s * d, 2048)
    g = torch.Generator().manual_seed(1)
    pp = dict(p)
    pp["image_prefix.proj.weight"] = torch.randn(s * d, 2048, generator=g) * 2048 ** -0.5
    pp["image_prefix.proj.bias"] = torch.randn(s * d, generator=g) * 0.02
    pp["image_prefix.ln.weight"] = 1.0 + torch.randn(d, generator=g) * 0.05
    pp["image_prefix.ln.bias"] = torch.randn(d, generator=g) * 0.02
    with torch.no_grad():
        ip.proj.weight.copy_(pp["image_prefix.proj.weight"]); ip.proj.bias.copy_(pp["image_prefix.proj.bias"])
        ip.ln.weight.copy_(pp["image_prefix.ln.weight"]); ip.ln.bias.copy_(pp["image_prefix.ln.bias"])
    ip.invalidate_packed()
    ip.eval()
    with torch.no_grad():
        ref2 = pooled_prefix_fwd(pp, d, s, ref)
        ppb = bf16_params(pp)
        eb2 = rel(pooled_prefix_fwd(ppb, d, s, encoder_fwd(ppb, c, x.to(BF16))), ref2)
        got2 = ip(x.cuda())
    assert got2.shape == (2, s, d)
    assert rel(got2, ref2) <= 2 * eb2 + 5e-3, (rel(got2, ref2), eb2)


def test_magma_with_nfresnet50_encoder(dev):
    """Magma built from a config that selects encoder_name "nfresnet50": checkpoint keys load by name, embed() yields
    image_seq_len prefix tokens per image, generate() runs; training the prefix + adapters on the frozen encoder steps."""
    from magma_amd.config import MultimodalConfig
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.nfnet import NFResNetConfig, init_params
    cfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name="nfresnet50", image_seq_len=4, image_size=128,
                           freeze_img_encoder=True, adapter_config={"mlp": {"adapter_type": "normal", "downsample_factor": 4}})
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=512, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=128)
    model = Magma(cfg, device=dev, lm_config=lm_cfg)
    missing, unexpected = model.load_checkpoint_state(init_params(NFResNetConfig(), seed=5))
    assert not unexpected and not any(k.startswith("image_prefix.enc.") for k in missing), (missing[:4], unexpected[:4])
    model.eval()
    assert model.image_prefix.pooled and model.image_prefix_seq_len == 4
    emb = model.embed([torch.randn(2, 3, 128, 128), torch.randint(0, 1000, (2, 5))])
    assert emb.shape == (2, 4 + 5, 512) and bool(torch.isfinite(emb.float()).all())
    toks = model.generate(emb, max_steps=3, temperature=0.0, decode=False, stop_on_eos=False)
    assert toks.shape == (2, 9 + 3)
    # the transform of the non-CLIP encoders (reference transforms.py:65-84) feeds it
    import numpy as np
    import PIL.Image as I
    img = model.transforms(I.fromarray(np.random.default_rng(0).integers(0, 256, (200, 300, 3), dtype=np.uint8)))
    assert img.shape == (1, 3, 128, 128) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    # frozen encoder: prefix + adapters train on top of it
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    caps = torch.full((2, model.seq_len), model.eos_token, dtype=torch.int64)
    caps[:, :9] = torch.randint(0, 1000, (2, 9))
    out = eng(torch.randn(2, 3, 128, 128).to(dev), caps.to(dev))
    eng.backward(out.loss)
    eng.step()
    assert bool(torch.isfinite(out.loss))


def test_nfnet_backward_kernels(dev):
    """weight_standardize_bwd / maxpool / subsample / relu-mean backward kernels against autograd on the same operands."""
    import torch.nn.functional as F
    from magma_amd import ops
    from oracle.nfnet import RELU_GAMMA, standardized_weight
    g = torch.Generator().manual_seed(2)
    for cout, cin, k in [(64, 3, 7), (48, 64, 1), (32, 24, 3)]:
        w = (torch.randn(cout, cin, k, k, generator=g) + 0.4).to(BF16)
        gain = (1 + 0.2 * torch.randn(cout, 1, 1, 1, generator=g)).to(BF16)
        fan_in = cin * k * k
        ld = (fan_in + 15) // 8 * 8
        dwh = torch.zeros(cout, ld)
        dwh[:, :fan_in] = torch.randn(cout, fan_in, generator=g)
        wf, gf = w.float().requires_grad_(True), gain.float().requires_grad_(True)
        (standardized_weight(wf, gf, 1e-5).reshape(cout, -1) * dwh[:, :fan_in] * 0.7).sum().backward()
        dw = torch.zeros(cout, fan_in, device=dev)
        dg = torch.zeros(cout, device=dev)
        ops.weight_standardize_bwd(w.cuda(), gain.cuda().reshape(-1), dwh.cuda(), dw, dg, RELU_GAMMA * fan_in ** -0.5, 1e-5, dmult=0.7)
        assert rel(dw, wf.grad.reshape(cout, -1)) < 2e-4 and rel(dg, gf.grad.reshape(-1)) < 2e-4
    x = torch.randn(2, 16, 10, 14, generator=g).to(BF16)
    dy = torch.randn(2, 16, 5, 7, generator=g).to(BF16)
    xf = x.float().requires_grad_(True)
    F.max_pool2d(xf, 3, stride=2, padding=1).backward(dy.float())
    got = ops.maxpool3x3s2_bwd(x.permute(0, 2, 3, 1).contiguous().cuda(), dy.permute(0, 2, 3, 1).contiguous().cuda())
    assert rel(got.permute(0, 3, 1, 2), xf.grad) < 4e-3          # bf16 rounding of sums of up to 4 window gradients
    ups = ops.subsample2_bwd(dy.permute(0, 2, 3, 1).contiguous().cuda(), 10, 14).permute(0, 3, 1, 2).cpu()
    ref = torch.zeros(2, 16, 10, 14, dtype=BF16)
    ref[:, :, ::2, ::2] = dy
    assert torch.equal(ups, ref)
    feats = torch.randn(2, 16, generator=g).to(BF16)
    xf = x.float().requires_grad_(True)
    (F.relu(xf).mean(dim=(2, 3)) * feats.float()).sum().backward()
    got = ops.relu_mean_rows_bwd(x.permute(0, 2, 3, 1).reshape(2, 140, 16).contiguous().cuda(), feats.cuda())
    assert rel(got.view(2, 10, 14, 16).permute(0, 3, 1, 2), xf.grad) < 4e-3


def nfresnet50_train_gradients(dev, image_hw, bf16_onednn=True):
    """Body of test_nfresnet50_train_gradients at an image of image_hw = (H, W); bf16_onednn=False runs the eager-bf16 baseline
    through PyTorch's native CPU convolution (tests/test_nonsquare_images_gpu.py: ONEDNN_BF16_WRONG).

    Training with encoder_name "nfresnet50" and the encoder UNFROZEN (the reference's default freeze_img_encoder: false):
    loss and the gradient of every trainable tensor -- all 53 scaled-std convs (weight, bias, gain, through the weight
    standardisation), the pooled prefix Linear + LayerNorm, the LM adapters -- against autograd through the fp32 oracle
    (oracle/nfnet.py: parity unpinned to timm, see its header).  Tolerance as tests/test_train_gpu.py."""
    import torch.nn.functional as F
    from magma_amd.config import MultimodalConfig
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import OracleConfig, build_labels, init_params as init_lm, lm_forward, pooled_prefix_fwd
    from oracle.nfnet import NFResNetConfig, encoder_fwd, init_params
    s_img, d, res = 2, 512, max(image_hw)
    mcfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name="nfresnet50", image_seq_len=s_img, image_size=res,
                            freeze_img_encoder=False, use_image_embed_layernorm=True, image_embed_dropout_prob=0.1,
                            adapter_config={"mlp": {"adapter_type": "normal", "downsample_factor": 4}},
                            image_enc_lr=2.0e-6, lr_decay_iters=1000)
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=d, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=128)
    model = Magma(mcfg, device=dev, lm_config=lm_cfg)
    cfg, c = OracleConfig.tiny(n_positions=128), NFResNetConfig()
    params = {k: t for k, t in init_lm(cfg, seed=31).items() if not k.startswith("image_prefix.")}
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    params.update(init_params(c, seed=5))
    g = torch.Generator().manual_seed(9)
    params["image_prefix.proj.weight"] = torch.randn(s_img * d, 2048, generator=g) * 2048 ** -0.5
    params["image_prefix.proj.bias"] = torch.randn(s_img * d, generator=g) * 0.02
    params["image_prefix.ln.weight"] = 1.0 + torch.randn(d, generator=g) * 0.05
    params["image_prefix.ln.bias"] = torch.randn(d, generator=g) * 0.02
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing[:4], unexpected[:4])
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    B, S = 2, model.seq_len
    images = torch.randn(B, 3, *image_hw, generator=g).to(BF16).float()
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    mask = (torch.rand(B, s_img, d, generator=g) < 0.9).float() / 0.9
    names = [k for k in params if ".adapter." in k or k.startswith("image_prefix.")]

    def oracle(dtype):
        p = {k: (t.detach().to(dtype).clone() if t.is_floating_point() else t) for k, t in params.items()}
        for k in names:
            p[k].requires_grad_(True)
        prefix = pooled_prefix_fwd(p, d, s_img, encoder_fwd(p, c, images.to(dtype)), dropout_mask=mask.to(dtype))
        labels = build_labels(s_img, caps, cfg.eos_token)
        words = F.embedding(caps, p["lm.transformer.wte.weight"]).to(prefix.dtype)
        out = lm_forward(p, cfg, inputs_embeds=torch.cat((prefix, words[:, : S - s_img, :]), dim=1), labels=labels)
        out["loss"].backward()
        return float(out["loss"].detach()), {k: p[k].grad.float() for k in names}

    loss_ref, g_ref = oracle(torch.float32)
    with contextlib.nullcontext() if bf16_onednn else torch.backends.mkldnn.flags(enabled=False):
        loss_bf, g_bf = oracle(BF16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref), (float(out.loss), loss_ref, loss_bf)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen, bad, worst = set(), [], []
    dots = n1 = n2 = bd = b1 = 0.0
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            got, ref, gb = eng.grad_of(p).float().cpu().reshape(-1), g_ref[n].reshape(-1), g_bf[n].reshape(-1)
            e_hip, e_bf = rel(got, ref), rel(gb, ref)
            worst.append((e_hip - 2 * e_bf, n, e_hip, e_bf))
            if e_hip > 2 * e_bf + 3e-2:
                bad.append((n, e_hip, e_bf))
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
            bd += float((gb * ref).sum()); b1 += float((gb * gb).sum())
    worst.sort(reverse=True)
    print("nf train: loss", float(out.loss), loss_ref, loss_bf, "| worst:", [(n, f"{a:.2e}", f"{b:.2e}") for _, n, a, b in worst[:5]])
    assert len(seen) == len(g_ref) and len(seen) > 160, (len(seen), len(g_ref), sorted(set(g_ref) - seen)[:5])
    assert not bad, bad[:8]
    cos_hip, cos_bf = dots / (n1 ** 0.5 * n2 ** 0.5), bd / (b1 ** 0.5 * n2 ** 0.5)
    assert 1 - cos_hip <= 2 * (1 - cos_bf) + 1e-3, (cos_hip, cos_bf)
    eng.step()
    eng.eval()
    assert torch.isfinite(eng(images.to(dev), caps.to(dev)).loss)



# ---------------------------------------------------------------------------------------------------------------------------
# the nine entry points of csrc/nfnet.hip, per element, at their edges (references and bounds: tests/kernel_compare.py)
#
# Every kernel here but the two weight-standardisation ones walks its elements with a grid-stride loop that takes a second
# trip only above 1 048 560 workgroups (host_grid): 2.7e8 elements, out of reach of a test that runs in seconds.  That branch
# is not covered.
# ---------------------------------------------------------------------------------------------------------------------------
MAPS = [(1, 1), (1, 7), (2, 2), (7, 9), (10, 14), (13, 13)]
CHANNELS, BATCHES = (8, 24, 64), (1, 3)
map_ids = lambda hw: f"{hw[0]}x{hw[1]}"           # noqa: E731


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def pool_input(kind, B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g)
    if kind == "normal":
        return z.to(BF16)
    if kind == "negative":                 # every border window then shows a padding of 0 instead of -inf
        return (-z.abs() - 1).to(BF16)
    if kind == "ties":                     # {-1, 0, 1}: most windows hold their maximum more than once
        return torch.randint(-1, 2, (B, C, H, W), generator=g).to(BF16)
    if kind == "constant":
        return torch.full((B, C, H, W), 0.5, dtype=BF16)
    if kind == "-inf":
        return torch.full((B, C, H, W), float("-inf"), dtype=BF16)
    if kind == "nan":                      # per image: one NaN and up to five -inf among normal values
        x = z.to(BF16).reshape(B, -1)
        for b in range(B):
            pos = torch.randperm(x.shape[1], generator=g)[:6]
            x[b, pos[1:]] = float("-inf")
            x[b, pos[0]] = float("nan")
        return x.reshape(B, C, H, W)
    raise ValueError(kind)


def same_with_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def tied_fraction(x):
    """Fraction of the 3x3 / stride-2 / padding-1 windows of x [B, C, H, W] whose maximum occurs more than once."""
    import torch.nn.functional as F
    xf = x.float()
    cols = F.unfold(F.pad(xf, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(x.shape[0], x.shape[1], 9, -1)
    return float(((cols == cols.amax(2, keepdim=True)).sum(2) > 1).float().mean())


@pytest.mark.parametrize("hw", MAPS, ids=map_ids)
def test_maxpool3x3s2_is_max_pool2d(dev, hw):
    """maxpool3x3s2 == F.max_pool2d(x, 3, 2, 1) bit for bit: odd maps (Ho = (H - 1) / 2 + 1), one-row and one-column maps,
    borders whose windows are all negative, ties, and PyTorch's special values: a NaN anywhere in a window is the result,
    -inf is an ordinary (smallest) value."""
    import torch.nn.functional as F
    from magma_amd import ops
    H, W = hw
    for C in CHANNELS:
        for B in BATCHES:
            for kind in ("normal", "negative", "ties", "nan", "-inf"):
                x = pool_input(kind, B, C, H, W, seed=H * 100 + W + C + B)
                want = F.max_pool2d(x.float(), 3, stride=2, padding=1)
                got = nchw(ops.maxpool3x3s2(nhwc(x))).float()
                assert got.shape == want.shape == (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
                if kind == "nan":
                    assert int(torch.isnan(want).sum()) >= B
                assert same_with_nan(got, want), (kind, B, C, H, W)


@pytest.mark.parametrize("hw", MAPS, ids=map_ids)
def test_maxpool3x3s2_bwd_ties_and_special_values(dev, hw):
    """maxpool3x3s2_bwd against the backward of F.max_pool2d (kernel_compare.maxpool3x3s2_bwd_reference): the gradient of a
    window goes to its FIRST maximum in a row-major scan that starts at the first valid entry and moves on where
    (v > best) || isnan(v).  Inputs with engineered ties -- a constant map (every window a full tie), {-1, 0, 1} -- an all -inf
    map (the gradient goes to the first valid entry) and NaN.  Up to four windows meet in one element: fp32 sum, one rounding;
    where one window contributes the result is dy's bits."""
    import torch.nn.functional as F
    from magma_amd import ops
    import kernel_compare as kcmp
    H, W = hw
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    worst = 0.0
    for C in CHANNELS:
        for B in BATCHES:
            for kind in ("normal", "constant", "ties", "-inf", "nan"):
                x = pool_input(kind, B, C, H, W, seed=H * 100 + W + C + B)
                if H * W > 1 and kind in ("constant", "-inf"):
                    assert tied_fraction(x) == 1.0
                if kind == "ties" and min(H, W) >= 7:       # windows of 2 .. 4 entries (narrow maps) tie less often
                    assert tied_fraction(x) >= 0.5, tied_fraction(x)
                dy = torch.randn(B, C, Ho, Wo, generator=torch.Generator().manual_seed(C + B)).to(BF16)
                ref, bound, cnt = kcmp.maxpool3x3s2_bwd_reference(x, dy)
                got = nchw(ops.maxpool3x3s2_bwd(nhwc(x), nhwc(dy)))
                worst = max(worst, kcmp.assert_elementwise(got, ref, bound, f"maxpool3x3s2_bwd {kind} {(B, C, H, W)}"))
                one = cnt == 1
                assert torch.equal(got[one].float().double(), ref[one]) and bool((got[cnt == 0] == 0).all())
                if kind == "normal":       # the reference IS autograd's backward (fp32 sums of the same window gradients)
                    xf = x.float().requires_grad_(True)
                    F.max_pool2d(xf, 3, stride=2, padding=1).backward(dy.float())
                    assert torch.allclose(ref, xf.grad.double(), rtol=1e-6, atol=1e-7)
    print(f"maxpool3x3s2_bwd {hw}: worst err/bound {worst:.3g}")
    if hw == (7, 9):
        # the pattern of the first valid window entries, written out: all-ones dy on a constant 5 x 7 map
        x, dy = torch.full((1, 8, 5, 7), 0.5, dtype=BF16), torch.ones(1, 8, 3, 4, dtype=BF16)
        got = nchw(ops.maxpool3x3s2_bwd(nhwc(x), nhwc(dy))).float()
        want = torch.zeros(5, 7)
        want[0] = want[1] = want[3] = torch.tensor([1.0, 1, 0, 1, 0, 1, 0])
        assert torch.equal(got, want.expand(1, 8, 5, 7))
        x[:] = float("-inf")
        assert torch.equal(nchw(ops.maxpool3x3s2_bwd(nhwc(x), nhwc(dy))).float(), want.expand(1, 8, 5, 7))


@pytest.mark.parametrize("hw", MAPS, ids=map_ids)
def test_subsample2_and_its_scatter(dev, hw):
    from magma_amd import ops
    H, W = hw
    for C in CHANNELS:
        for B in BATCHES:
            x = pool_input("normal", B, C, H, W, seed=H + W + C + B)
            sub = nchw(ops.subsample2(nhwc(x)))
            assert torch.equal(sub, x[:, :, ::2, ::2])
            up = nchw(ops.subsample2_bwd(nhwc(sub), H, W))
            want = torch.zeros_like(x)
            want[:, :, ::2, ::2] = sub
            assert torch.equal(up, want)
            off = torch.ones(H, W, dtype=torch.bool)
            off[::2, ::2] = False
            assert bool((up[:, :, off] == 0).all()) and not bool(torch.signbit(up[:, :, off]).any())


@pytest.mark.parametrize("C,k,stride,pad,H,W,ldo", [(3, 7, 2, 3, 17, 23, 160), (3, 3, 2, 1, 9, 9, 32), (8, 1, 1, 0, 5, 6, 8),
                                                      (4, 3, 1, 1, 6, 5, 48)])
def test_im2col_nchw_is_unfold(dev, C, k, stride, pad, H, W, ldo):
    import torch.nn.functional as F
    from magma_amd import ops
    K = C * k * k
    for B in BATCHES:
        img = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(K + B)).to(BF16)
        cols = ops.im2col_nchw(img.cuda(), k, stride, pad, ldo).cpu()
        ref = F.unfold(img.float(), k, padding=pad, stride=stride).transpose(1, 2).reshape(-1, K)      # column (c, ky, kx)
        assert cols.shape == (ref.shape[0], ldo)
        assert torch.equal(cols[:, :K].float(), ref)
        assert bool((cols[:, K:] == 0).all()) and not bool(torch.signbit(cols[:, K:]).any())


WS_SHAPES = [(64, 3, 7), (40, 24, 3), (16, 3, 3), (8, 2048, 1), (8, 512, 3)]       # (16, 3, 3): fan-in 27 under 256 threads


@pytest.mark.parametrize("cout,cin,k", WS_SHAPES)
def test_weight_standardize_per_element(dev, cout, cin, k):
    """Both column orders, ldo = fan-in and larger, and the three row kinds of kernel_compare.standardize_rows against
    kernel_compare.weight_standardize_reference.  A constant row is 0 within the cancellation term; an all-zero row exactly 0."""
    from magma_amd import ops
    import kernel_compare as kcmp
    from oracle.nfnet import RELU_GAMMA, standardized_weight
    fan_in = cin * k * k
    scale = RELU_GAMMA * fan_in ** -0.5
    worst = 0.0
    for kind in kcmp.WS_ROW_KINDS:
        w, gain = kcmp.standardize_rows(kind, cout, cin, k, seed=cout + fan_in)
        for khwc in (False, True):
            ref, bound = kcmp.weight_standardize_reference(w, gain, scale, 1e-5, to_khwc=khwc)
            for ldo in (fan_in, (fan_in + 15) // 8 * 8):
                got = ops.weight_standardize(w.cuda(), gain.cuda(), scale, 1e-5, to_khwc=khwc, ldo=ldo).cpu()
                assert got.shape == (cout, ldo) and bool((got[:, fan_in:] == 0).all())
                worst = max(worst, kcmp.assert_elementwise(got[:, :fan_in], ref, bound, f"weight_standardize {kind} {(cout, cin, k)} khwc={khwc} ldo={ldo}"))
                if kind == "constant":
                    assert float(ref.abs().max()) == 0.0 and bool((got[0] == 0).all()) and bool((got[-1] == 0).all())
        if kind == "normal":       # the fp64 reference states what the oracle states
            assert rel(kcmp.weight_standardize_reference(w, gain, scale, 1e-5)[0], standardized_weight(w.float(), gain.float(), 1e-5).reshape(cout, -1)) < 1e-5
    print(f"weight_standardize {(cout, cin, k)}: worst err/bound {worst:.3g}")


@pytest.mark.parametrize("cout,cin,k", WS_SHAPES)
def test_weight_standardize_bwd_per_element(dev, cout, cin, k):
    """dw / dgain against the closed form of the kernel's header in fp64 (kernel_compare.weight_standardize_bwd_reference;
    tests/test_kernel_compare_cpu.py checks that form against autograd).  The kernel ACCUMULATES: both buffers start non-zero and
    the start is subtracted in fp64.  dwhat has a padded leading dimension whose padding holds NaN; dmult != 1; constant and
    all-zero rows give finite results."""
    from magma_amd import ops
    import kernel_compare as kcmp
    from oracle.nfnet import RELU_GAMMA
    fan_in = cin * k * k
    scale = RELU_GAMMA * fan_in ** -0.5
    ld = (fan_in + 15) // 8 * 8
    worst = {"dw": 0.0, "dgain": 0.0}
    for kind in kcmp.WS_ROW_KINDS:
        w, gain = kcmp.standardize_rows(kind, cout, cin, k, seed=cout + fan_in + 1)
        g = torch.Generator().manual_seed(fan_in)
        dwh = torch.full((cout, ld), float("nan"))
        dwh[:, :fan_in] = torch.randn(cout, fan_in, generator=g)
        dw0, dg0 = torch.randn(cout, fan_in, generator=g), torch.randn(cout, generator=g)
        dw, dg = dw0.cuda(), dg0.cuda()
        ops.weight_standardize_bwd(w.cuda(), gain.cuda(), dwh.cuda(), dw, dg, scale, 1e-5, dmult=0.7)
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(dg).all())
        R = kcmp.weight_standardize_bwd_reference(w.reshape(cout, -1), gain, dwh[:, :fan_in], scale, 1e-5, 0.7, dw0, dg0)
        worst["dw"] = max(worst["dw"], kcmp.assert_elementwise(dw.cpu().double() - dw0.double(), *R["dw"], f"weight_standardize_bwd dw {kind} {(cout, cin, k)}"))
        worst["dgain"] = max(worst["dgain"], kcmp.assert_elementwise(dg.cpu().double() - dg0.double(), *R["dgain"], f"weight_standardize_bwd dgain {kind} {(cout, cin, k)}"))
    print(f"weight_standardize_bwd {(cout, cin, k)}: worst err/bound dw {worst['dw']:.3g}, dgain {worst['dgain']:.3g}")


RM_C, RM_HW = (2, 16, 64, 66, 130, 2048), (1, 9, 31, 32, 33, 49, 140)      # 66, 130: a ragged last 64-channel slab; 31 / 32 / 33: the 32 position slices


@pytest.mark.parametrize("C", RM_C)
def test_relu_mean_rows_per_element(dev, C):
    from magma_amd import ops
    import kernel_compare as kcmp
    worst, n_tiny = {"fwd": 0.0, "bwd": 0.0}, 0
    for HW in RM_HW:
        for B in BATCHES:
            x, g = kcmp.relu_rows_input(B, HW, C, seed=C + HW + B)
            ref, bound = kcmp.relu_mean_rows_reference(x)
            got = ops.relu_mean_rows(x.cuda()).cpu()
            worst["fwd"] = max(worst["fwd"], kcmp.assert_elementwise(got, ref, bound, f"relu_mean_rows {(B, HW, C)}"))
            neg = ops.relu_mean_rows((-x.abs() - 1).cuda()).cpu()
            assert bool((neg == 0).all()) and not bool(torch.signbit(neg).any())           # all negative: exactly +0
            ref, bound = kcmp.relu_mean_rows_bwd_reference(x, g)
            dx = ops.relu_mean_rows_bwd(x.cuda(), g.cuda()).cpu()
            closed = x <= 0
            assert bool((dx[closed] == 0).all()), "the gate is x > 0: +0 and -0 close it"
            tiny = x == 2.0 ** -133
            n_tiny += int(tiny.sum())
            assert bool((dx[tiny] != 0).all()), "the smallest positive bf16 opens it"
            worst["bwd"] = max(worst["bwd"], kcmp.assert_elementwise(dx, ref, bound, f"relu_mean_rows_bwd {(B, HW, C)}"))
    assert n_tiny > 0
    print(f"relu_mean_rows C={C}: worst err/bound forward {worst['fwd']:.3g}, backward {worst['bwd']:.3g}")


def test_nfnet_kernels_refuse_bad_shapes(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    x = torch.zeros(1, 4, 4, 12, dtype=BF16, device=dev)                 # C = 12: not a multiple of 8
    for fn in (ops.maxpool3x3s2, ops.subsample2, lambda t: ops.subsample2_bwd(t, 8, 8)):
        with pytest.raises(MagmaHipError):
            fn(x)
    with pytest.raises(MagmaHipError):
        ops.relu_mean_rows(torch.zeros(1, 4, 7, dtype=BF16, device=dev))  # odd C
    img = torch.zeros(1, 3, 8, 8, dtype=BF16, device=dev)
    for ldo in (24, 28, 36):                                              # K = 27: ldo < K; ldo % 8 != 0 (below and above K)
        with pytest.raises(MagmaHipError):
            ops.im2col_nchw(img, 3, 2, 1, ldo)
    w = torch.zeros(8, 3, 3, 3, dtype=BF16, device=dev)
    with pytest.raises(MagmaHipError):
        ops.weight_standardize(w, torch.ones(8, dtype=BF16, device=dev), 1.0, 1e-5, ldo=26)


def test_nfresnet50_train_gradients(dev):
    nfresnet50_train_gradients(dev, (128, 128))
