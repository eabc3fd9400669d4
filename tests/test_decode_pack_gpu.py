"""Lossless decode packing (MAGMA_DECODE_PACK): bf16 weights streamed as 13.25-bit twins (low byte, 4-bit offset of e>>1 against a
per-block base, sign) that the weight-streaming GEMVs widen back to the SAME bf16 bits in registers.  Nothing here has a tolerance:
pack -> inverse is compared bit for bit on the CPU, and on the GPU every packed launch must equal the bf16 launch of the same
operands under torch.equal -- the MFMA operands, their order and the cross-wave sum are those of the bf16 kernel with the same waves."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BF16 = torch.bfloat16
gpu = pytest.mark.gpu


def hint(waves, kc, nt):
    return nt | waves << 4 | kc << 8


def rnd(*shape, dev="cpu", scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def bits(t):
    return t.contiguous().view(torch.int16)


def misfit_tiles(w):
    """Brute force, independent of the packer: the 16-row tiles of a bf16 [n16, K] that hold a 32-element block whose (e>>1) values
    span more than 15."""
    eh = ((bits(w).to(torch.int32) >> 8) & 0x7f).view(w.shape[0], w.shape[1] // 32, 32)
    bad = (eh.amax(-1) - eh.amin(-1)) > 15
    return bad.view(w.shape[0] // 16, 16, -1).any(2).any(1)


def roundtrip(w):
    """pack -> inverse: the flags must be exactly the misfit tiles, every row of every other tile bit-exact.  Returns the flags."""
    from magma_amd import ops
    lo, nib, base, sign, flags = ops.pack_bf16_lossless(w)
    nt, K = w.shape[0] // 16, w.shape[1]
    assert lo.shape == (nt, K // 64, 4, 16, 2, 8) and nib.shape == (nt, K // 128, 4, 16, 4, 4)
    assert base.shape == (nt, K // 128, 16) and sign.shape == (nt, K // 128, 4, 16) and base.dtype == sign.dtype == torch.int32
    assert flags.dtype == torch.uint8 and flags.numel() % 16 == 0 and not flags[nt:].any()
    bytes_streamed = sum(t.numel() * t.element_size() for t in (lo, nib, base, sign))
    assert bytes_streamed * 8 == w.numel() * 13.25
    want = misfit_tiles(w)
    assert torch.equal(flags[:nt].bool(), want)
    back = ops.unpack_bf16_lossless(lo, nib, base, sign)
    keep = (~want).repeat_interleave(16)
    assert torch.equal(bits(back)[keep], bits(w)[keep])
    return flags[:nt].bool()


# ------------------------------------------------------------------------------------------------------------ the format (CPU)
def test_gaussian_weights_roundtrip():
    w = rnd(256, 1024, scale=0.02, seed=1).to(BF16)
    flags = roundtrip(w)
    assert flags.sum() <= 1, "N(0, 0.02) blocks almost always fit (about 1.5 in a million do not)"


def test_every_bf16_bit_pattern_roundtrips():
    """All 65 536 patterns -- zeros, denormals, Inf, NaN, both signs -- three times: in counting order (a block shares its high
    byte: every tile fits), shuffled inside the eight windows of 16 consecutive e>>1 values (every block mixes signs, offsets and
    low bytes and still fits: all 65 536 patterns come back exactly), and shuffled freely (misfit tiles: flagged)."""
    idx = torch.arange(65536, dtype=torch.int32)
    pat = idx.to(torch.int16).view(BF16)
    assert not roundtrip(pat.view(512, 128).clone()).any()
    perm = torch.randperm(65536, generator=torch.Generator().manual_seed(2))
    window = ((idx >> 8) & 0x7f) >> 4                                   # 8192 patterns = 64 whole rows per window
    order = perm[torch.argsort(window[perm], stable=True)]
    assert not roundtrip(pat[order].view(512, 128).clone()).any()
    assert roundtrip(pat[perm].view(512, 128).clone()).any()


def test_all_zero_block_fits():
    from magma_amd import ops
    w = torch.zeros(16, 128, dtype=BF16)
    assert not roundtrip(w).any()
    w[:, 32:64] = -0.0                                # a block of negative zeros: sign bits only
    w[3, 64:96] = rnd(32, scale=0.02, seed=3).to(BF16)  # zeros in OTHER blocks of the row do not matter
    assert not roundtrip(w).any()
    w[3, 70] = 0.0                                    # an exact zero beside normal values does
    assert roundtrip(w).all()
    pk = ops.DecodePack(ops.PackedLinear.tile(w))
    assert pk.escaped == 1 and pk.ntiles == 1


# ------------------------------------------------------------------------------------------------------------ the kernel
def make_linear(dev, N, K, escapes, seed):
    """(bf16 PackedLinear without a twin, the same operand with a twin whose bf16 copy is ZEROED in every tile that is not escaped,
    flags).  A packed launch that read W where it should read the planes -- or the planes of an escaped tile -- cannot produce
    the reference bits from that operand."""
    from magma_amd import ops
    w = rnd(N, K, scale=0.02, seed=seed)
    w = torch.where(w.abs() < 1e-5, torch.full_like(w, 1e-5), w).to(BF16)      # no accidental misfit: |w| in [1e-5, ~0.1]
    nt = (N + 15) // 16
    if escapes == "planted":
        w[0, 5] = 0.0                                   # an exact zero in tile 0
        if nt > 1:
            w[17, 40] = w[17, 40] * 2.0 ** -40          # a 2^-40-scaled element in tile 1
    elif escapes == "all":
        for t in range(nt):
            w[16 * t + (3 * t) % min(16, N - 16 * t), 32 * t + 7] = 0.0
    bias = rnd(N, seed=seed + 1).to(dev)
    ref = ops.PackedLinear(w.to(dev), bias=bias)
    lin = ops.PackedLinear(w.to(dev), bias=bias)
    pk = ops.attach_decode_pack(lin)
    assert pk is not None and lin.pk is pk
    flags = pk.flags[:nt].bool()
    want = {"none": [False] * nt, "all": [True] * nt, "planted": ([True, True] + [False] * nt)[:nt]}[escapes]
    assert flags.tolist() == want, (flags.tolist(), want)
    lin.ft = lin.ft.clone()
    lin.ft[~flags] = 0
    return ref, lin, flags


def epilogues(dev, M, N, K, ref):
    """The epilogues of the token step, as keyword arguments of gemm_skinny: the dec_in form (LayerNorm fold, two segments, GELU on
    the second), ReLU (adapter-down), two residuals ([W_out | W_up]), fp32 logits behind a LayerNorm fold (head)."""
    from magma_amd import ops
    colsum = ops.PackedLinear.untile(ref.ft)[:N].float().sum(1).contiguous()
    r0, r1 = rnd(M, N, dev=dev, seed=21).to(BF16), rnd(M, N, dev=dev, seed=22).to(BF16)
    out = {"relu": dict(act=ops.MG_ACT_RELU),
           "res2": dict(residuals=(r0, r1)),
           "logits": dict(out_dtype=torch.float32, ln_fold=(colsum, K, 1e-5))}
    if N > 16:
        nb = N - 16
        out["dec_in"] = dict(ln_fold=(colsum, K, 1e-5),
                             split=(16, lambda: torch.empty(M, ops.ceil_to(nb, 8), dtype=BF16, device=dev)[:, :nb],
                                    ops.MG_ACT_GELU_NEW, rnd(nb, dev=dev, seed=23)))
    else:
        out["dec_in"] = dict(ln_fold=(colsum, K, 1e-5), act=ops.MG_ACT_GELU_NEW)
    return out


def run(x, lin, kw, variant=0):
    """gemm_skinny with a fresh second-segment buffer; returns every output tensor."""
    from magma_amd import ops
    kw = dict(kw)
    outs = []
    if "split" in kw:
        n0, mk, act, bias_b = kw["split"]
        ob = mk()
        kw["split"] = (n0, ob, act, bias_b)
        outs.append(ob)
        lin = _first_segment(lin, n0)
    out = ops.gemm_skinny(x, lin, variant=variant, **kw)
    outs.insert(0, out[:, : kw["split"][0]] if "split" in kw else out)      # a split launch writes the first segment's columns only
    return outs


def _first_segment(lin, n0):
    from magma_amd import ops
    v = ops.PackedLinear.__new__(ops.PackedLinear)
    v.__dict__.update(lin.__dict__)
    v.bias = lin.bias[:n0].contiguous()
    return v


# (waves, kc) of the packed variants against the bf16 variant with the same waves
PACKED_VARIANTS = {1024: [(0, 0), (hint(8, 4, 1), 0), (hint(8, 4, 2), 0), (hint(4, 4, 1), hint(4, 1, 1)), (hint(4, 8, 1), hint(4, 1, 1))],
                   5120: [(0, 0), (hint(8, 4, 1), 0), (hint(8, 4, 2), 0), (hint(8, 20, 1), 0), (hint(4, 8, 1), hint(4, 1, 1))]}


@gpu
@pytest.mark.parametrize("escapes", ["planted", "all", "none"])
@pytest.mark.parametrize("K", [1024, 5120])
def test_gemv_packed_equals_bf16(dev, K, escapes):
    """M in {1, 8, 16} x N in {16, 40, 48} (40: a ragged last tile) x every epilogue of the step; K = 1024 / 5120 give the 8-wave
    kernel 1 / 5 k-step quads per wave.  Escapes: an exact zero in tile 0 and a 2^-40-scaled element in tile 1 | every tile | none."""
    for N in (16, 40, 48):
        ref, lin, flags = make_linear(dev, N, K, escapes, seed=N + K)
        for M in (1, 8, 16):
            x = (rnd(M, K, dev=dev, seed=M + K) * 2 + 0.3).to(BF16)
            for name, kw in epilogues(dev, M, N, K, ref).items():
                for v_pk, v_bf in PACKED_VARIANTS[K]:
                    want, got = run(x, ref, kw, v_bf), run(x, lin, kw, v_pk)
                    for a, b in zip(want, got):
                        assert a.dtype == b.dtype and torch.equal(a, b), (N, M, name, hex(v_pk), (a != b).nonzero()[:4])
                if M == 8 and name == "relu" and not flags.all():     # the zeroed bf16 copy is visible to a bf16 launch
                    assert not torch.equal(run(x, ref, kw)[0], _bf16_launch(x, lin, kw))


def _bf16_launch(x, lin, kw):
    from magma_amd import ops
    v = ops.PackedLinear.__new__(ops.PackedLinear)
    v.__dict__.update(lin.__dict__)
    v.pk = None
    return run(x, v, kw)[0]


@gpu
def test_every_packed_variant(dev):
    """K = 4096 (16 / 32 k-steps per wave with 8 / 4 waves): every instantiated (waves, burst, n-tiles) against the bf16 launch with
    the same waves, N = 72 (five tiles: a ragged last workgroup for two tiles per workgroup), escapes planted."""
    N, K, M = 72, 4096, 8
    ref, lin, _ = make_linear(dev, N, K, "planted", seed=7)
    x = rnd(M, K, dev=dev, seed=8).to(BF16)
    kw = dict(out_dtype=torch.float32)
    want = {8: run(x, ref, kw, hint(8, 4, 1))[0], 4: run(x, ref, kw, hint(4, 1, 1))[0]}
    assert torch.equal(run(x, ref, kw)[0], want[8])
    for waves, kc, nt in [(8, 4, 1), (8, 4, 2), (8, 8, 1), (8, 8, 2), (8, 16, 1), (4, 4, 1), (4, 8, 1), (4, 16, 1), (4, 16, 2), (4, 32, 1)]:
        assert torch.equal(run(x, lin, kw, hint(waves, kc, nt))[0], want[waves]), (waves, kc, nt)

@gpu
def test_refusals(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    _, lin, _ = make_linear(dev, 40, 1024, "none", seed=9)
    x = rnd(4, 1024, dev=dev).to(BF16)
    call = lambda d: ops.check(ops.L.load().mg_gemm_skinny_bf16(ops.C.byref(d), ops._stream()), "mg_gemm_skinny_bf16")  # noqa: E731
    with pytest.raises(MagmaHipError):          # pipelined bursts are bf16-only
        ops.gemm_skinny(x, lin, variant=hint(8, 4, 1) | 1 << 16)
    with pytest.raises(MagmaHipError):          # 16 waves: 2 k-steps per wave, no whole quad
        ops.gemm_skinny(x, lin, variant=hint(16, 2, 1))
    with pytest.raises(MagmaHipError):          # a burst that is no whole number of quads
        ops.gemm_skinny(x, lin, variant=hint(4, 2, 1))
    d, _ = ops.skinny_desc(x, lin)
    d.pk_sign = None                            # all five planes or none
    with pytest.raises(MagmaHipError):
        call(d)
    d, _ = ops.skinny_desc(x, lin)
    d.pk_base = lin.pk.base.data_ptr() + 4      # misaligned plane
    with pytest.raises(MagmaHipError):
        call(d)
    assert ops.attach_decode_pack(ops.PackedLinear(rnd(32, 768, dev=dev).to(BF16))) is None      # K % 512: no twin


@gpu
def test_pair_and_attention_co_launch(dev, monkeypatch):
    """gemm_skinny2 and attention || GEMV at K = 2048 with a short cache: packed against the bf16 launch of the same call -- both
    GEMV outputs, the context rows and the appended cache."""
    from magma_amd import ops
    from oracle.model import rotary_tables
    K = 2048
    ra, la, _ = make_linear(dev, 72, K, "planted", seed=31)
    rb, lb, _ = make_linear(dev, 40, 1024, "none", seed=32)
    xa, xb = rnd(8, K, dev=dev, seed=33).to(BF16), rnd(8, 1024, dev=dev, seed=34).to(BF16)

    def pair(a, b):
        oa = torch.empty(8, 72, dtype=BF16, device=dev)
        ob = torch.empty(8, 40, dtype=torch.float32, device=dev)
        ops.gemm_skinny2((xa, a, oa, {}), (xb, b, ob, {"act": ops.MG_ACT_RELU}))
        return oa, ob
    for got, want in zip(pair(la, lb), pair(ra, rb)):
        assert torch.equal(got, want)
    B, H, Smax, rot = 3, 4, 128, 64
    d = H * 256
    kc0 = rnd(B, H, Smax, 256, dev=dev, seed=11, scale=0.5).to(BF16)
    vc0 = rnd(B, H, Smax, 256, dev=dev, seed=12).to(BF16)
    qkv = rnd(B, 3 * d, dev=dev, seed=13, scale=0.5).to(BF16)
    sin_t, cos_t = (t.to(dev).contiguous() for t in rotary_tables(rot, Smax))
    d_pos = torch.tensor([20], dtype=torch.int32, device=dev)
    xg = rnd(B, K, dev=dev, seed=14).to(BF16)

    def co(lin):
        kc, vc, ctx = kc0.clone(), vc0.clone(), torch.empty(B, d, dtype=BF16, device=dev)
        y = torch.empty(B, 72, dtype=BF16, device=dev)
        ops.decode_attn_gemv(qkv, kc, vc, ctx, B, H, d_pos, rot, sin_t, cos_t, (xg, lin, y, {}))
        return kc, vc, ctx, y
    for got, want in zip(co(la), co(ra)):
        assert torch.equal(got, want)
    assert torch.equal(co(la)[3], ops.gemm_skinny(xg, ra, variant=hint(4, 1, 1)))
    monkeypatch.setattr(ops, "DECODE_PACK", False)             # the switch: la's zeroed bf16 copy is what streams now
    assert not torch.equal(co(la)[3], co(ra)[3])


# ------------------------------------------------------------------------------------------------------------ the engine
N_STEPS = 6


def _model(dev, monkeypatch, pack):
    """Two blocks, d 1024 (4 heads of 256), ff 2048, adapter bottleneck 512: the smallest width at which every operand of the
    "fold2" block packs (K = 1024, 2048, 1024, 1536 and the head's 1024 are multiples of 512; at d = 256 no K is)."""
    from magma_amd.testing import build_reduced_magma
    monkeypatch.setenv("MAGMA_DECODE_PACK", "1" if pack else "0")
    torch.manual_seed(0)
    model = build_reduced_magma(dev, n_layer=2, n_head=4, d_ff=2048, mlp_factor=2)
    model.eval()
    assert model.lm.engine.decode_pack == pack
    return model


def _emb(model, B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, model.lm.config.hidden_size, generator=g).to(BF16).to(model.device)


def _captured_steps(model, emb, n):
    eng = model.lm.engine
    eng._cache_pool.clear()
    o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=n + 1)
    tok = o.logits[:, -1].argmax(-1, keepdim=True)
    logits = []
    for _ in range(n):
        lg = eng.decode(tok, o.past_key_values)[0].float().clone()     # use_graph: captured on the first call, replayed after
        logits.append(lg)
        tok = lg.argmax(-1, keepdim=True)
    st = o.past_key_values.decode_state
    assert st.kinds == ["fold2"] * 2 and st.refusal is None
    return torch.stack(logits)


@gpu
def test_engine_mode_on_equals_mode_off(dev, monkeypatch):
    from magma_amd import ops
    emb = None
    res = {}
    for pack in (True, False):
        model = _model(dev, monkeypatch, pack)
        emb = _emb(model, 3, 7, seed=51) if emb is None else emb
        with torch.no_grad():
            steps = _captured_steps(model, emb, N_STEPS)
            ids = model.generate(emb, max_steps=N_STEPS, temperature=0.0, decode=False, stop_on_eos=False).cpu()
        eng = model.lm.engine
        twins = [getattr(p, "pk", None) for ly in eng.layers for p in (ly.dec_in, ly.fc_out, ly.mlp_adapter[0], ly.out_up)] + \
                [getattr(eng.head_dec, "pk", None)]
        assert all((t is not None) == pack for t in twins), twins
        res[pack] = (steps, ids)
        if pack:
            assert eng.decode_pack_share() >= 0.97
            # an in-place adapter write, then repack_adapters: the rebuilt operands have new twins, and the packed step equals the
            # bf16 step of the same engine again
            old = eng.layers[0].out_up.pk
            with torch.no_grad():
                for name, p in model.lm.named_parameters():
                    if ".adapter." in name and name.endswith("weight"):
                        p.mul_(1.5)
                eng.repack_adapters(model.lm)
                assert eng.layers[0].out_up.pk is not None and eng.layers[0].out_up.pk is not old
                assert eng.layers[0].mlp_adapter[0].pk is not None and eng.layers[0].dec_in.pk is twins[0]
                after = _captured_steps(model, emb, 2)
                monkeypatch.setattr(ops, "DECODE_PACK", False)
                after_bf16 = _captured_steps(model, emb, 2)
                monkeypatch.setattr(ops, "DECODE_PACK", True)
            assert torch.equal(after, after_bf16) and not torch.equal(after[0], steps[0])
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
