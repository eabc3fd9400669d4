"""Batch generation over prompts of different lengths (ragged batches, right padding; DESIGN.md "Ragged batches").

  * the decode kernels with one KV write position per row (pos_stride = 1) against a PyTorch fp32 statement of every row;
  * the bookkeeping launches advancing every row's position;
  * on the reduced model: equal lengths through the ragged path are bit-identical to the uniform path, the padding does not
    leak into any row (zero padding == random padding, bit for bit), in every decode configuration (grouped v1 / v2 steps,
    fold modes 0 / 1 / 2, the B > 16 tile-GEMM step, W8A16, sampled mode, multi-token input_ids on a ragged cache);
  * the public API: Magma.embed_batch, generate(..., lengths=) and its output layout, and the error cases."""
import math

import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def assert_close(got, ref, tol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    e = float((got - ref).norm() / (ref.norm() + 1e-12))
    assert math.isfinite(e) and e < tol, f"{what}: rel-L2 {e:.3e} >= {tol}"


# ------------------------------------------------------------------------------------------------------------ kernels
def test_decode_kernels_per_row_positions(dev):
    from magma_amd import ops
    from oracle.model import apply_rotary, rotary_tables
    B, H, Smax, rot = 5, 2, 320, 64
    pos = [3, 17, 64, 129, 300]
    d = H * 256
    kc0 = rnd(B, H, Smax, 256, dev=dev, seed=11, scale=0.5).to(BF16)
    vc0 = rnd(B, H, Smax, 256, dev=dev, seed=12).to(BF16)
    qkv = rnd(B, 3 * d, dev=dev, seed=13, scale=0.5).to(BF16)
    sin_t, cos_t = rotary_tables(rot, Smax)
    sin_t, cos_t = sin_t.to(dev).contiguous(), cos_t.to(dev).contiguous()
    d_pos = torch.tensor(pos, dtype=torch.int32, device=dev)
    x = qkv.view(B, 3, H, 256).float().cpu()

    kc, vc = kc0.clone(), vc0.clone()
    out = torch.empty(B, d, dtype=BF16, device=dev)
    ops.attn_decode_fused(qkv, kc, vc, out, B, H, d_pos, rot, sin_t, cos_t, pos_stride=1)
    q_rot = []
    for b, p in enumerate(pos):
        pt = torch.tensor([p])
        k_new = apply_rotary(x[b:b + 1, 1][:, None], pt, rot)[0, 0]          # (H, 256) at row b's own position
        q_rot.append(apply_rotary(x[b:b + 1, 0][:, None], pt, rot)[0, 0])
        assert_close(kc[b, :, p], k_new, 3e-3, f"appended k, row {b}")
        assert torch.equal(vc[b, :, p].float().cpu(), x[b, 2]), f"appended v, row {b}"
        keep = torch.ones(Smax, dtype=torch.bool)
        keep[p] = False
        assert torch.equal(kc[b][:, keep], kc0[b][:, keep]) and torch.equal(vc[b][:, keep], vc0[b][:, keep]), f"row {b}: other slots"
        sc = (q_rot[-1][:, None, :] @ kc[b, :, : p + 1].float().cpu().transpose(-1, -2)) / 16.0
        ref = (torch.softmax(sc, -1) @ vc[b, :, : p + 1].float().cpu()).reshape(d)
        assert_close(out[b], ref, 3e-3, f"fused decode attention, row {b}")
    # per element, on the bf16 q the kernel itself attends with (the stand-alone rotary pass writes the same q, k, v bits)
    qk = torch.empty(B, H, 1, 256, dtype=BF16, device=dev)
    kcx, vcx = kc0.clone(), vc0.clone()
    ops.rotary_split(qkv, B, 1, H, rot, sin_t, cos_t, qk, kcx, vcx, d_pos=d_pos, pos_stride=1)
    assert torch.equal(kcx, kc) and torch.equal(vcx, vc)
    kcmp.assert_causal_attention(out, qk, kc, vc, f"fused decode attention, positions {pos}", p0=d_pos, p_dtype=torch.float32, n_rescale=0)

    # stand-alone attention on an already rotated q, over the cache the fused launch wrote
    q = torch.stack(q_rot).to(BF16).to(dev).view(B, H, 1, 256).contiguous()
    out2 = torch.empty(B, d, dtype=BF16, device=dev)
    ops.attn_decode(q, kc, vc, out2, B, H, d_pos, pos_stride=1)
    for b, p in enumerate(pos):
        sc = (q[b].float().cpu() @ kc[b, :, : p + 1].float().cpu().transpose(-1, -2)) / 16.0
        ref = (torch.softmax(sc, -1) @ vc[b, :, : p + 1].float().cpu()).reshape(d)
        assert_close(out2[b], ref, 3e-3, f"decode attention, row {b}")
    kcmp.assert_causal_attention(out2, q, kc, vc, f"decode attention, positions {pos}", p0=d_pos, p_dtype=torch.float32, n_rescale=0)

    # the co-launch with a GEMV: the same attention body, so the same cache writes and the same context rows
    kc3, vc3 = kc0.clone(), vc0.clone()
    out3 = torch.empty(B, d, dtype=BF16, device=dev)
    xg = rnd(B, 1024, dev=dev, seed=14).to(BF16)
    w = rnd(512, 1024, dev=dev, seed=15, scale=0.05).to(BF16)
    lin = ops.PackedLinear(w)
    y = torch.empty(B, 512, dtype=torch.float32, device=dev)
    ops.decode_attn_gemv(qkv, kc3, vc3, out3, B, H, d_pos, rot, sin_t, cos_t, (xg, lin, y, {"out_dtype": torch.float32}),
                         pos_stride=1)
    assert torch.equal(kc3, kc) and torch.equal(vc3, vc)
    assert torch.equal(out3, out)
    assert_close(y, xg.float() @ w.float().t(), 1e-3, "co-launched GEMV")
    kcmp.assert_linear(y, "co-launched GEMV (per-row positions)", xg, w)
    assert d_pos.tolist() == pos, "the decode kernels must not move the positions"

    # pos_stride 0 on the same buffer: every row appends at d_pos[0], as before
    kc4, vc4 = kc0.clone(), vc0.clone()
    ops.attn_decode_fused(qkv, kc4, vc4, torch.empty_like(out), B, H, d_pos, rot, sin_t, cos_t)
    assert torch.equal(vc4[:, :, pos[0]].float().cpu(), x[:, 2]) and torch.equal(vc4[1:, :, pos[1]], vc0[1:, :, pos[1]])


def test_bookkeeping_advances_every_row(dev):
    from magma_amd import ops
    pos = [3, 17, 64, 129, 300]
    p = torch.tensor(pos, dtype=torch.int32, device=dev)
    ops.advance_pos(p, 2, pos_stride=1)
    assert p.tolist() == [v + 2 for v in pos]
    ops.advance_pos(p, 1)                                   # shared position: entry 0 only
    assert p.tolist() == [pos[0] + 3] + [v + 2 for v in pos[1:]]
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    hist = torch.zeros(5, 4, dtype=torch.int64, device=dev)
    tok = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int64, device=dev)
    p = torch.tensor(pos, dtype=torch.int32, device=dev)
    ops.sample_finish(tok, 9, state, d_pos=p, delta=1, history=hist, pos_stride=1)
    assert p.tolist() == [v + 1 for v in pos] and state.tolist() == [1, -1] and hist[:, 0].tolist() == [1, 2, 3, 4, 5]
    ops.sample_finish(tok, 9, state, d_pos=p, delta=3)      # shared position: entry 0 only
    assert p.tolist() == [pos[0] + 4] + [v + 1 for v in pos[1:]]
    with pytest.raises(ValueError):
        ops.advance_pos(p, 1, pos_stride=2)
    with pytest.raises(ValueError):
        ops.sample_finish(torch.zeros(8, dtype=torch.int64, device=dev), 9, state, d_pos=p, pos_stride=1)   # 5 positions, B = 8


# ------------------------------------------------------------------------------------------------------- the engine
def _model(dev, **kw):
    from magma_amd.testing import build_reduced_magma
    torch.manual_seed(kw.pop("seed", 3))
    model = build_reduced_magma(dev, **kw)
    model.eval()
    return model


def _teacher_forced(model, emb, lengths, ids, sampling=None):
    """prefill + len(ids) cached steps on the given ids: (prefill logits, [step logits], [step tokens]) as host copies."""
    kw = {} if lengths is None else {"lengths": lengths}
    out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=ids.shape[1] + 4, **kw)
    cache = out.past_key_values
    logits, toks = [out.logits[:, -1].float().cpu()], []
    for i in range(ids.shape[1]):
        o = model.lm(input_ids=ids[:, i:i + 1], use_cache=True, past_key_values=cache, sampling=sampling)
        logits.append(o.logits[:, -1].float().cpu())
        toks.append(o.next_token.cpu().clone())
    return logits, toks, cache


def _ragged_embeds(model, B, S, seed, pad_noise: bool, lengths):
    """(B, S, d) embeddings, row b valid on [0, len_b) (drawn from ``seed``); the padding is zeros or, with ``pad_noise``,
    large random finite values -- the valid part is the same either way."""
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(B, S, model.lm.config.hidden_size, generator=g) * 0.5).to(BF16)
    noise = torch.randn(B, S, model.lm.config.hidden_size, generator=torch.Generator().manual_seed(seed + 1)).to(BF16)
    for b, n in enumerate(lengths):
        emb[b, n:] = noise[b, n:] * 3.0 if pad_noise else 0
    return emb.to(model.device)


def _check_uniform_and_leak(model, B, S, lengths, steps=5, sampling=None):
    dev = model.device
    V = model.lm.config.vocab_size
    ids = torch.randint(0, min(V, 1000), (B, steps), generator=torch.Generator().manual_seed(7)).to(dev)
    # equal lengths through the ragged path == the uniform path, bit for bit
    emb = _ragged_embeds(model, B, S, 1, False, [S] * B)
    a = _teacher_forced(model, emb, None, ids, sampling)
    b = _teacher_forced(model, emb, [S] * B, ids, sampling)
    assert b[2].ragged and not a[2].ragged
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"uniform vs ragged(equal lengths): logits of step {i}"
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    # zero padding vs random finite padding: every row, every step identical
    z = _teacher_forced(model, _ragged_embeds(model, B, S, 2, False, lengths), lengths, ids, sampling)
    r = _teacher_forced(model, _ragged_embeds(model, B, S, 2, True, lengths), lengths, ids, sampling)
    for i, (x, y) in enumerate(zip(z[0], r[0])):
        assert torch.isfinite(x).all() and torch.equal(x, y), f"padding leaks into the logits of step {i}"
    for x, y in zip(z[1], r[1]):
        assert torch.equal(x, y)
    assert z[2].d_pos.tolist() == [n + steps for n in lengths] and z[2].pos == max(lengths) + steps
    return z


@pytest.mark.parametrize("config", ["v1", "v2"])
def test_uniform_lengths_bit_identical_and_padding_does_not_leak(dev, config):
    model = _model(dev, attn_factor=8 if config == "v2" else None)
    _check_uniform_and_leak(model, 4, 23, [23, 9, 16, 1])
    # generate(): uniform lengths through the ragged path give the same tokens
    emb = _ragged_embeds(model, 3, 12, 5, False, [12] * 3)
    a = model.generate(emb, max_steps=6, temperature=0.0, stop_on_eos=False, decode=False)
    b = model.generate(emb, max_steps=6, temperature=0.0, stop_on_eos=False, decode=False, lengths=[12] * 3)
    assert torch.equal(a, b)


@pytest.mark.parametrize("fold", ["0", "1"])
def test_fold_modes(dev, monkeypatch, fold):
    monkeypatch.setenv("MAGMA_DECODE_FOLD", fold)
    model = _model(dev)
    assert model.lm.engine.fold_dn == int(fold)
    _check_uniform_and_leak(model, 3, 17, [5, 17, 11])


def test_wide_batch_tile_gemm_step(dev):
    model = _model(dev)
    lengths = [3 + (7 * b) % 18 for b in range(20)]
    lengths[4] = 20
    with pytest.warns(RuntimeWarning):
        _check_uniform_and_leak(model, 20, 20, lengths, steps=3)


def test_w8a16_decode(dev, monkeypatch):
    # d 4096 (16 heads), adapter bottleneck 1024: every decode operand has an e4m3 copy (K % 1024 == 0)
    monkeypatch.setenv("MAGMA_DECODE_W8", "1")
    model = _model(dev, n_layer=1, n_head=16, d_ff=4096, vocab=1056)
    assert model.lm.engine.decode_w8
    _check_uniform_and_leak(model, 3, 14, [14, 6, 10], steps=3)


def test_sampled_mode(dev):
    model = _model(dev)
    mode = (0.9, 20, 0.9)
    B, S, lengths = 3, 15, [15, 4, 9]
    _check_uniform_and_leak(model, B, S, lengths, steps=4, sampling=mode)
    emb = _ragged_embeds(model, B, S, 9, False, lengths)
    kw = dict(max_steps=8, temperature=0.9, top_k=20, top_p=0.9, decode=False, stop_on_eos=False)
    a = model.generate(emb, seed=123, lengths=lengths, **kw)
    b = model.generate(emb, seed=123, lengths=lengths, **kw)
    c = model.generate(emb, seed=124, lengths=lengths, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # graph replay == eager launches of the same token step
    eng = model.lm.engine
    out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=8, sampling=mode, eos_token=model.eos_token, seed=123,
                   lengths=lengths)
    toks, cache = [out.next_token.clone()], out.past_key_values
    for _ in range(7):
        _, tk = eng.decode(toks[-1][:, None], cache, use_graph=False, sampling=mode)
        toks.append(tk.clone())
    toks = torch.stack(toks, 1)
    for b_, n in enumerate(lengths):
        assert torch.equal(a[b_, n:n + 8], toks[b_])
    # the stream is keyed by (seed, step, row): equal lengths through the ragged path draw what the uniform path draws
    emb_u = _ragged_embeds(model, B, S, 9, False, [S] * B)
    assert torch.equal(model.generate(emb_u, seed=5, **kw), model.generate(emb_u, seed=5, lengths=[S] * B, **kw))


def test_multi_token_input_ids_on_ragged_cache(dev):
    model = _model(dev)
    B, S, T, lengths = 3, 13, 4, [13, 2, 8]
    emb = _ragged_embeds(model, B, S, 3, False, lengths)
    ids = torch.randint(0, 1000, (B, T), generator=torch.Generator().manual_seed(1)).to(dev)
    o1 = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=T + 2, lengths=lengths)
    multi = model.lm(input_ids=ids, use_cache=True, past_key_values=o1.past_key_values)
    assert multi.logits.shape[:2] == (B, T)
    single, _, cache = _teacher_forced(model, emb, lengths, ids)
    for i in range(T):
        assert torch.equal(multi.logits[:, i].float().cpu(), single[i + 1]), f"position {i}"
    assert torch.equal(o1.past_key_values.d_pos, cache.d_pos)


# ------------------------------------------------------------------------------------------------------- public API
def test_embed_batch_and_generate(dev, tmp_path):
    from PIL import Image
    from magma_amd import ImageInput
    model = _model(dev)
    paths = []
    for i in range(3):
        arr = (torch.rand(80, 96, 3, generator=torch.Generator().manual_seed(i)) * 255).to(torch.uint8).numpy()
        p = tmp_path / f"img{i}.png"
        Image.fromarray(arr).save(p)
        paths.append(str(p))
    qs = ["short q", "a much longer question about what is in the picture, with detail", "mid-size question"]
    batch = [[ImageInput(paths[i]), qs[i]] for i in range(3)]
    batch.append(["text only, no image at all"])
    snapshot = [list(s) for s in batch]
    emb, lengths = model.embed_batch(batch)
    assert all(a == b for sa, sb in zip(batch, snapshot) for a, b in zip(sa, sb)) and all(len(a) == len(b) for a, b in zip(batch, snapshot))
    singles = [model.embed(model.preprocess_inputs(list(s), embed=False)) for s in batch]
    assert lengths.tolist() == [e.shape[1] for e in singles]
    assert emb.shape == (4, max(lengths.tolist()), model.lm.config.hidden_size)
    for b, e in enumerate(singles):
        n = int(lengths[b])
        assert bool((emb[b, n:] == 0).all()), f"row {b}: padding must be zeros"
        assert_close(emb[b, :n], e[0], 2e-2, f"row {b} vs embed() of the sample alone")
        text_rows = n if b == 3 else model.tokenizer.encode(qs[b], return_tensors="pt").shape[1]
        assert torch.equal(emb[b, n - text_rows:n], e[0, n - text_rows:n]), f"row {b}: text embeddings"
    # every image went through ONE image_prefix call: the image rows are those of the batched call
    imgs = torch.cat([ImageInput(p).get_transformed_image(model.transforms) for p in paths])
    pre = model.image_prefix(imgs.to(dev))
    for b in range(3):
        assert torch.equal(emb[b, : pre.shape[1]], pre[b])

    n = 6
    strs = model.generate(emb, max_steps=n, temperature=0.0, lengths=lengths)
    assert isinstance(strs, list) and len(strs) == 4 and all(isinstance(s, str) for s in strs)
    toks = model.generate(emb, max_steps=n, temperature=0.0, lengths=lengths, decode=False, stop_on_eos=False)
    S = emb.shape[1]
    assert toks.shape == (4, S + n)
    for b in range(4):
        lb = int(lengths[b])
        assert bool((toks[b, :lb] == model.image_token).all())
        assert bool((toks[b, lb + n:] == model.eos_token).all())
    # a list of per-sample embeddings is padded internally
    toks2 = model.generate([emb[b:b + 1, : int(lengths[b])] for b in range(4)], max_steps=n, temperature=0.0, decode=False,
                           stop_on_eos=False)
    assert torch.equal(toks, toks2)
    # the generated tokens of row b are those of the sample alone (teacher-forced check of the first step: prefill logits)
    o = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=4, lengths=lengths)
    for b in range(4):
        lb = int(lengths[b])
        alone = model.lm(inputs_embeds=emb[b:b + 1, :lb], use_cache=True, cache_hint=4)
        assert_close(o.logits[b, -1], alone.logits[0, -1], 1e-2, f"row {b} prefill logits vs the sample alone")


def test_error_cases(dev):
    model = _model(dev)
    emb = _ragged_embeds(model, 3, 10, 1, False, [10, 5, 7])
    kw = dict(max_steps=2, temperature=0.0, decode=False)
    for bad in ([10, 0, 7], [10, 11, 7], [10, 5], [[10, 5, 7]]):
        with pytest.raises(ValueError):
            model.generate(emb, lengths=bad, **kw)
        with pytest.raises(ValueError):
            model.lm(inputs_embeds=emb, use_cache=True, lengths=bad)
    with pytest.raises(TypeError):
        model.generate(emb, lengths=[10.0, 5.0, 7.0], **kw)
    with pytest.raises(ValueError):                    # lengths only at the prefill
        model.lm(inputs_embeds=emb, use_cache=False, lengths=[10, 5, 7])
    # cache overflow: a ragged cache refuses the step past its last slot
    o = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=1, lengths=[10, 5, 7])
    cache = o.past_key_values
    assert cache.Smax == 64 and cache.pos == 10
    ids = torch.zeros(3, cache.Smax - cache.pos + 1, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="KV cache full"):
        model.lm(input_ids=ids, use_cache=True, past_key_values=cache)
    assert int(cache.d_pos.max()) == cache.Smax and cache.d_pos.tolist() == [64, 59, 61]

    # an LM object without the engine rejects lengths instead of attending over the padding
    class HostLM(torch.nn.Module):
        device_token_selection = False

        def forward(self, **kw):
            raise AssertionError("must not be called")
    real = model.lm
    try:
        model.lm = HostLM()
        with pytest.raises(ValueError, match="HIP engine"):
            model.generate(emb, lengths=[10, 5, 7], **kw)
    finally:
        model.lm = real
