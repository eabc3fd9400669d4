"""Non-square images through the two convolutional image encoders.

Both encoders take any (B, 3, H, W) with H and W multiples of 32 and thread (h, w) by hand through every NHWC view, pool,
implicit-im2col argument and backward tape (image_encoders.py, train_engine.py).  On a square image an h / w mix-up at any of
those sites computes the same thing; here H != W, forward and backward, against the CPU oracle with the tolerance of the
square tests.  32 x 128 and 128 x 32 end in 1 x 4 and 4 x 1 maps: the 3x3 implicit im2col and the 2x2 average pool on one-row
and one-column maps.

Each size is checked together with its spatial transpose: the oracle's output for the transposed image must be far (ten
tolerances) from the HIP output, so an encoder that read the image with its sides swapped could not pass."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SIZES = [(32, 128), (128, 32), (64, 96)]


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def bf16_params(p):
    return {k: (v.to(BF16) if v.is_floating_point() else v) for k, v in p.items()}


# The eager-bf16 baseline is PyTorch's CPU convolution in bf16.  Its oneDNN path is wrong for NF-ResNet's last strided conv at
# 128 x 32 -- 3x3, stride 2, padding 1, [2, 512, 8, 2] -> [2, 512, 4, 1]: rel-L2 1.28 against the fp32 convolution of the same
# operands where every other shape gives 1.7e-3, and the whole encoder then returns NaN or a 0.12 error from run to run
# (torch 2.10 CPU).  A tolerance made of that is no tolerance: at this size the baseline runs with oneDNN off (0.017, in line
# with 0.015 / 0.016 at the other two sizes).  The fp32 oracle, which is the reference, is not affected.
ONEDNN_BF16_WRONG = ((128, 32),)
_images = {}


def image(hw):
    """The bf16-exact test image of a size; 128 x 32 is the transpose of 32 x 128 and 96 x 64 that of 64 x 96, so that the
    oracle runs once per size and serves as 'the other orientation' of its transpose.

    Content with an orientation: every row has a level of its own (N(0, 1) per image, channel and row) under N(0, 0.5) noise, so
    the transposed image has column stripes.  With white noise alone the trunks' pooling averages the input away and the two
    orientations differ by 0.18 .. 0.22 (CLIP trunk) and 0.31 .. 0.44 (NF-ResNet, a global mean) of the oracle's output: about
    ten tolerances, too close to call.  With the stripes the oracle's two outputs are 0.32 .. 0.44 and 0.74 .. 1.07 apart."""
    if not _images:
        for i, (h, w) in enumerate([(32, 128), (64, 96)]):
            g = torch.Generator().manual_seed(40 + i)
            x = (torch.randn(2, 3, h, 1, generator=g).expand(2, 3, h, w) + 0.5 * torch.randn(2, 3, h, w, generator=g)).to(BF16).float()
            _images[(h, w)] = x
            _images[(w, h)] = x.transpose(2, 3).contiguous()
    return _images[hw]


class Oracle:
    """fp32 and eager-bf16 outputs of an oracle encoder per image size, computed once.  ``no_onednn``: sizes whose eager-bf16
    run goes through PyTorch's native CPU convolution (see ONEDNN_BF16_WRONG)."""

    def __init__(self, fwd, params, cfg, no_onednn=()):
        self.fwd, self.p, self.pb, self.cfg, self.ref, self.eb = fwd, params, bf16_params(params), cfg, {}, {}
        self.no_onednn = no_onednn

    def reference(self, hw):
        if hw not in self.ref:
            with torch.no_grad():
                self.ref[hw] = self.fwd(self.p, self.cfg, image(hw))
        return self.ref[hw]

    def eager_bf16_error(self, hw):
        if hw not in self.eb:
            with torch.no_grad(), torch.backends.mkldnn.flags(enabled=False) if hw in self.no_onednn else contextlib.nullcontext():
                self.eb[hw] = rel(self.fwd(self.pb, self.cfg, image(hw).to(BF16)), self.reference(hw))
        return self.eb[hw]


def check_orientation(enc, oracle, hw, transposed_like):
    """HIP against the oracle at one size (HIP rel-L2 <= 2 x eager-bf16 rel-L2 + 5e-3), and the oracle's output for the
    transposed image -- brought to the layout of this one by ``transposed_like`` -- more than ten tolerances away."""
    x = image(hw)
    ref = oracle.reference(hw)
    got = enc(x.cuda())
    tol = 2 * oracle.eager_bf16_error(hw) + 5e-3
    other = transposed_like(oracle.reference((hw[1], hw[0])))
    print(f"{type(enc).__name__} @{hw}: HIP {rel(got, ref):.3e}, tolerance {tol:.3e}, oracle of the transposed image {rel(other, ref):.3e} "
          f"(HIP against it {rel(got, other):.3e})")
    assert got.shape == ref.shape
    assert rel(got, ref) <= tol, (rel(got, ref), tol)
    assert rel(other, ref) > 10 * tol and rel(got, other) > 10 * tol, (rel(other, ref), rel(got, other), tol)
    return got


@pytest.fixture(scope="module")
def clip(dev):
    """The reduced model of tests/test_model_gpu.py::setup, variant v1."""
    from magma_amd.testing import build_reduced_magma
    from oracle.model import OracleConfig, encoder_fwd, init_params
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=0)
    params = init_params(cfg, seed=11)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    model = build_reduced_magma(dev, mlp_factor=4, attn_factor=None)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected, unexpected
    model.eval()
    return model, Oracle(encoder_fwd, params, cfg), cfg


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clip_trunk_forward(clip, hw):
    """(B, (H/32) (W/32), d) tokens in "b (h w) d" order.  The transposed image's tokens come in "b (w h) d" order: as a
    (w, h) grid transposed back they are this image's tokens had the trunk been symmetric -- it is not."""
    model, oracle, cfg = clip
    h, w = hw[0] // 32, hw[1] // 32

    def transposed_like(t):
        return t.view(t.shape[0], w, h, -1).transpose(1, 2).reshape(t.shape[0], h * w, -1)
    got = check_orientation(model.image_prefix.enc, oracle, hw, transposed_like)
    assert got.shape == (2, {(32, 128): 4, (128, 32): 4, (64, 96): 6}[hw], 32 * cfg.enc_width)


@pytest.fixture(scope="module")
def nfnet(dev):
    """NF-ResNet-50 as tests/test_nfresnet_gpu.py::test_nfresnet50_encoder_and_pooled_prefix sets it up."""
    from magma_amd.image_encoders import NFResNet50
    from oracle.nfnet import NFResNetConfig, encoder_fwd, init_params
    c = NFResNetConfig()
    p = init_params(c, seed=3)
    enc = NFResNet50(128, device=dev, dtype=BF16)
    enc.load_state_dict({k[len("image_prefix.enc."):]: t for k, t in p.items()}, strict=True)
    enc.invalidate_packed()
    return enc, Oracle(encoder_fwd, p, c, no_onednn=ONEDNN_BF16_WRONG)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nfresnet50_forward(nfnet, hw):
    enc, oracle = nfnet
    with torch.no_grad():
        got = check_orientation(enc, oracle, hw, lambda t: t)
    assert got.shape == (2, 2048)


def test_clip_trunk_train_gradients_32x128(dev):
    """tests/test_train_gpu.py::test_gradients_and_step (v1, encoder unfrozen) at 32 x 128: 4 prefix tokens as at 64 x 64, from a
    1 x 4 final map -- the geom / out_geom tapes, avgpool2_bwd and im2col_t with h != w."""
    from test_train_gpu import gradients_and_step
    gradients_and_step(dev, "v1", image_hw=(32, 128))


def test_nfresnet50_train_gradients_128x32(dev):
    """tests/test_nfresnet_gpu.py::test_nfresnet50_train_gradients at 128 x 32: geom0 and the max-pool backward on a 64 x 16 map,
    subsample2_bwd(dy, H, W) and the avgpool2_bwd of the shortcut down to a 4 x 1 map."""
    from test_nfresnet_gpu import nfresnet50_train_gradients
    nfresnet50_train_gradients(dev, (128, 32), bf16_onednn=False)        # ONEDNN_BF16_WRONG
