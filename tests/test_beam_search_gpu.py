"""Beam search on the device (DESIGN.md "Beam search"): the per-row top-2k selection kernel, the bookkeeping launch and the
KV-cache reorder against host statements, and generate(num_beams=...) on the reduced model against the host statement of
the rule (magma_amd.sampling.beam_search, pinned to transformers by tests/test_beam_search_cpu.py) driven by the engine's
own decode logits, with an independent re-scoring of every returned hypothesis by the cache-less forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _gapped_logits(R, V, seed, gap=1e-3):
    """Row logits that are a random permutation of an evenly spaced grid: no ties, and any two scores of a row differ by
    >= gap, so the comparison with the float64 statement is exact whatever the rounding of the logsumexp."""
    g = torch.Generator().manual_seed(seed)
    base = torch.arange(V, dtype=torch.float64) * gap * 4
    rows = [base[torch.randperm(V, generator=g)] - 0.5 * V * gap * 4 + torch.randn(1, generator=g, dtype=torch.float64)
            for _ in range(R)]
    return torch.stack(rows).float()


@pytest.mark.parametrize("V", [1056, 50258])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_selection_kernel(dev, V, k):
    from magma_amd import ops
    B = 2
    R = B * k
    x = _gapped_logits(R, V, seed=V + k)
    g = torch.Generator().manual_seed(k)
    run = (torch.randn(R, generator=g) * 3 - 5).float()
    run.view(B, k)[0, 1:] = -1e9                   # sample 0 at its first step: beams 1.. must not expand
    ld = V + 7
    xd = torch.zeros(R, ld, device=dev)
    xd[:, :V] = x.to(dev)
    cs = torch.zeros(R, 2 * k, device=dev)
    ct = torch.zeros(R, 2 * k, dtype=torch.int32, device=dev)
    ops.beam_topk(xd[:, :V], run.to(dev), cs, ct)
    lp = torch.log_softmax(x.double(), -1) + run.double()[:, None]
    ref_s, ref_t = torch.topk(lp, 2 * k, dim=-1)
    live = run > -1e8                  # rows at -1e9: every fp32 score rounds to -1e9 (ties, ordered by token)
    assert torch.equal(ct.cpu().long()[live], ref_t[live])
    assert torch.allclose(cs.cpu().double()[live], ref_s[live], rtol=1e-6, atol=0)
    # fp32 there: -1e9 + lp rounds to -1e9 for every lp above -32, so the kernel's order is (fp32 score desc, token asc)
    sc32 = run[~live][:, None] + torch.log_softmax(x[~live], -1)
    order = torch.sort(-sc32, dim=-1, stable=True)[1][:, : 2 * k]
    assert bool((cs.cpu()[~live] == -1e9).all()) and torch.equal(ct.cpu()[~live].long(), order)
    # the per-sample merge inside the bookkeeping launch: parents and tokens of step 0 (no eos among them)
    st = _state(dev, B, k, ld=8)
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    ops.beam_finish(cs, ct, B, k, V, V + 100, 1.0, False, 50, state, st)
    flat = lp.view(B, k * V)
    top = torch.topk(flat, 2 * k, dim=-1)[1][:, :k]
    assert torch.equal(st["parent"].cpu().long().view(B, k), top // V + torch.arange(B)[:, None] * k)
    assert torch.equal(st["token"].cpu().view(B, k), top % V)
    if k > 1:
        assert bool((st["parent"].view(B, k)[0] == 0).all())


def _state(dev, B, k, ld, eos=0):
    R = B * k
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    run = z(R, dt=f32)
    run.view(B, k)[:, 1:] = -1e9
    return dict(run=run, fin_score=torch.full((R,), -1e9, device=dev), fin_flag=z(R, dt=i32), fin_len=z(R, dt=i32),
                fin_tok=torch.full((R, ld), eos, dtype=i64, device=dev), fin_stage=z(R, ld, dt=i64), hist=z(R, ld, dt=i64),
                hist_stage=z(R, ld, dt=i64), unsat=torch.ones(B, dtype=i32, device=dev), parent=z(R, dt=i32), token=z(R, dt=i64))


def _scripted(k, lp, es, eos_mode, B=3, V=64, n=10, eos=5):
    """Logits per step.  "random": eos boosted by a random amount per step (it lands among the first k and outside them,
    some hypotheses finish early, the others at max_steps).  "heavy": from step 1 on eos tops every row, so the slots fill
    within a few steps and generation stops before max_steps (except "never" with a positive length_penalty)."""
    R = B * k
    g = torch.Generator().manual_seed(100 * k + int(lp * 10) + len(str(es)))
    # a different spread per row and step: every row's log-probabilities differ from every other row's, so no two candidate
    # sums tie across beams (equal scores would be ordered by index here and in unspecified order by torch.topk)
    scale = 200 + 200 * torch.rand(n, R, 1, generator=g, dtype=torch.float64)
    table = [(_gapped_logits(R, V, seed=1000 + t).double() * scale[t]).float() for t in range(n)]
    for t in range(n):
        if eos_mode == "random":
            table[t][:, eos] += float(torch.rand(1, generator=g)) * 10 - 3
        elif t >= 1:
            table[t][:, eos] = table[t].max(-1).values + 1.0 + 5 * torch.rand(R, generator=g)
    return table


GRID = [(k, lp, es) for k in (1, 2, 4) for lp in (1.0, 0.0, 2.0, -0.5) for es in (True, False, "never")]


def _host_run(table, B, k, n, eos, lp, es):
    from magma_amd.sampling import beam_search
    parents, rec = [], []

    def step(rows, tokens):
        if rows is not None:
            parents.append(rows.clone())
        return table[len(parents)]

    return beam_search(step, B, k, n, eos, lp, es, k, record=rec), parents, rec


def test_scripted_fixtures_exercise_every_rule():
    """What the bookkeeping test relies on, over its grid: hypotheses that finish on eos among the first k before max_steps,
    eos candidates outside the first k, hypotheses that run to max_steps, and stops before max_steps with full slots under
    each early_stopping mode."""
    seen = set()
    for k, lp, es in GRID:
        for mode in ("random", "heavy"):
            (_, _, lens), _, rec = _host_run(_scripted(k, lp, es, mode), 3, k, 10, 5, lp, es)
            if any(bool((r["finished"] & (r["step"] + 1 < 10)).any()) for r in rec):
                seen.add("eos among the first k")
            if any(bool(r["eos_outside"].any()) for r in rec):
                seen.add("eos outside the first k")
            if bool((lens == 10).any()):
                seen.add("max_steps")
            if len(rec) < 10:
                seen.add(f"stop before max_steps, early_stopping={es}")
                assert mode == "heavy" or k == 1
    assert seen == {"eos among the first k", "eos outside the first k", "max_steps", "stop before max_steps, early_stopping=True",
                    "stop before max_steps, early_stopping=False", "stop before max_steps, early_stopping=never"}, seen


@pytest.mark.parametrize("eos_mode", ["random", "heavy"])
@pytest.mark.parametrize("k,lp,es", GRID)
def test_bookkeeping_against_host_rule(dev, k, lp, es, eos_mode):
    """The selection and bookkeeping launches against the host statement step for step on scripted logits; then two more
    steps past the recorded stop (the host reads it only every few steps) must leave every finished slot as it is."""
    from magma_amd import ops
    B, V, n, eos = 3, 64, 10, 5
    R = B * k
    table = _scripted(k, lp, es, eos_mode)
    (ref_seq, ref_sc, ref_len), host_parents, _ = _host_run(table, B, k, n, eos, lp, es)
    if eos_mode == "heavy" and not (es == "never" and lp > 0):
        assert len(host_parents) + 1 < n and bool((ref_len < n).all())
    st = _state(dev, B, k, ld=n + 4, eos=eos)
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    cs = torch.zeros(R, 2 * k, device=dev)
    ct = torch.zeros(R, 2 * k, dtype=torch.int32, device=dev)
    dev_parents = []
    for t in range(n):
        ops.beam_topk(table[t].to(dev), st["run"], cs, ct)
        ops.beam_finish(cs, ct, B, k, V, eos, lp, es, n, state, st)
        dev_parents.append(st["parent"].cpu().long())
        if int(state[1]) >= 0:
            break
    assert int(state[1]) == len(host_parents), (int(state[1]), len(host_parents))
    for a, b in zip(host_parents, dev_parents):
        assert torch.equal(a, b)
    lens = st["fin_len"].cpu().long()
    m = int(lens.max())
    assert torch.equal(lens, ref_len) and m == ref_seq.shape[1]
    assert torch.equal(st["fin_tok"].cpu()[:, :m], ref_seq)
    assert torch.allclose(st["fin_score"].cpu(), ref_sc, rtol=1e-6, atol=1e-6)
    assert bool(st["fin_flag"].bool().all())
    frozen = {name: st[name].clone() for name in ("fin_score", "fin_flag", "fin_len", "fin_tok", "unsat")}
    stop, t0 = int(state[1]), int(state[0])
    for t in range(t0, min(t0 + 2, n)):
        ops.beam_topk(table[t].to(dev), st["run"], cs, ct)
        ops.beam_finish(cs, ct, B, k, V, eos, lp, es, n, state, st)
        assert torch.equal(st["parent"].cpu(), torch.arange(R, dtype=torch.int32))
    assert int(state[1]) == stop and all(torch.equal(frozen[name], st[name]) for name in frozen)


@pytest.mark.parametrize("ragged", [False, True])
def test_kv_reorder_matches_index_select(dev, ragged):
    from magma_amd import ops
    L, R, H, Smax = 3, 6, 2, 40
    g = torch.Generator().manual_seed(7)
    maps = {"identity": [0, 1, 2, 3, 4, 5], "broadcast": [0, 0, 0, 3, 3, 3], "swap": [1, 0, 2, 4, 3, 5],
            "3-cycle": [1, 2, 0, 3, 5, 4], "mixed": [2, 2, 0, 5, 3, 3], "across lengths": [3, 1, 5, 0, 4, 2]}
    pos = [17, 17, 17, 33, 33, 33] if ragged else [25] * R
    d_pos = torch.tensor(pos if ragged else pos[:1], dtype=torch.int32, device=dev)
    for name, parent in maps.items():
        k0 = torch.randn(L, R, H, Smax, 256, generator=g).to(BF16).to(dev)
        v0 = torch.randn(L, R, H, Smax, 256, generator=g).to(BF16).to(dev)
        kc, vc = k0.clone(), v0.clone()
        ks, vs = torch.empty_like(kc), torch.empty_like(vc)
        par = torch.tensor(parent, dtype=torch.int32, device=dev)
        ops.kv_reorder(kc, vc, ks, vs, par, d_pos, pos_stride=1 if ragged else 0)
        idx = torch.tensor(parent, device=dev)
        kr, vr = k0.index_select(1, idx), v0.index_select(1, idx)
        for b in range(R):
            n = pos[parent[b]] if parent[b] != b else pos[b]        # row b receives the positions its parent holds
            assert torch.equal(kc[:, b, :, :n], kr[:, b, :, :n]) and torch.equal(vc[:, b, :, :n], vr[:, b, :, :n]), (name, b)
            assert torch.equal(kc[:, b, :, n:], k0[:, b, :, n:]) and torch.equal(vc[:, b, :, n:], v0[:, b, :, n:]), (name, b)


# ------------------------------------------------------------------------------------------------------- the reduced model
def _model(dev, monkeypatch=None, w8=False, **kw):
    from magma_amd.testing import build_reduced_magma
    if w8:
        monkeypatch.setenv("MAGMA_DECODE_W8", "1")
    torch.manual_seed(0)
    model = build_reduced_magma(dev, **kw)
    model.eval()
    with torch.no_grad():       # eos within reach, at different steps for different beams
        model.lm.lm_head.bias[model.eos_token] += 4.0
        model.lm.invalidate_packed()
    return model


def _emb(model, B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, model.lm.config.hidden_size, generator=g)).to(BF16).to(model.device)


def _host_on_engine(model, emb, k, n, lp, es, n_ret, lengths=None):
    """The host statement driven by the engine's own cached decode: cache rows reordered by index_select, greedy step, the
    logits of every row -- the same kernels, so the same logits for the same cache contents."""
    from magma_amd.sampling import beam_search
    eng = model.lm.engine
    emb_k = emb.repeat_interleave(k, dim=0)
    box = {}
    kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths).repeat_interleave(k)}

    def step(rows, tokens):
        if rows is None:
            o = eng.forward(inputs_embeds=emb_k, use_cache=True, cache_hint=n, **kw)
            box["c"] = o.past_key_values
            return o.logits[:, -1].float().cpu()
        c = box["c"]
        r = rows.to(model.device)
        c.k.copy_(c.k.index_select(1, r))
        c.v.copy_(c.v.index_select(1, r))
        lg, _ = eng.decode(tokens.view(-1, 1).to(model.device), c, use_graph=False)
        return lg.float().cpu()

    return beam_search(step, emb.shape[0], k, n, model.eos_token, lp, es, n_ret)


def _check_against_host(model, emb, k, n, lp=1.0, es=False, n_ret=None, lengths=None):
    n_ret = n_ret or k
    ref_seq, ref_sc, ref_len = _host_on_engine(model, emb, k, n, lp, es, n_ret, lengths)
    out, sc = model.generate(emb if lengths is None else emb, max_steps=n, num_beams=k, length_penalty=lp, early_stopping=es,
                             num_return_sequences=n_ret, decode=False, return_scores=True, lengths=lengths)
    S = emb.shape[1]
    assert out.shape == (emb.shape[0] * n_ret, S + ref_seq.shape[1])
    if lengths is None:
        got = out[:, S:].cpu()
    else:
        lr = torch.as_tensor(lengths).repeat_interleave(n_ret)
        got = torch.stack([out[i, int(lr[i]): int(lr[i]) + ref_seq.shape[1]].cpu() for i in range(out.shape[0])])
    assert torch.equal(got, ref_seq), (got, ref_seq)
    assert torch.allclose(sc, ref_sc, rtol=1e-5, atol=1e-5), (sc, ref_sc)
    return out, sc, ref_len


def test_num_beams_one_is_todays_greedy(dev):
    model = _model(dev)
    emb = _emb(model, 2, 6, seed=1)
    a = model.generate(emb, max_steps=8, temperature=0.0, decode=False)
    b = model.generate(emb, max_steps=8, temperature=0.0, decode=False, num_beams=1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("cfg", ["v1", "v2", "none", "w8", "ragged", "wide"])
def test_engine_beam_equals_host_statement(dev, monkeypatch, cfg):
    # W8A16 needs K % 1024 == 0 for every decode operand: d 4096 (16 heads), adapter bottleneck 1024, one block
    kw = {"v2": dict(attn_factor=8), "none": dict(mlp_factor=None, adapter_config=None),
          "w8": dict(n_layer=1, n_head=16, d_ff=4096)}.get(cfg, {})
    model = _model(dev, monkeypatch, w8=cfg == "w8", **kw)
    assert model.lm.engine.decode_w8 == (cfg == "w8")
    if cfg == "wide":
        B, k = 5, 4                               # 20 rows: the eager tile-GEMM step
    else:
        B, k = 3, 4
    emb = _emb(model, B, 7, seed=20 + len(cfg))
    lengths = [7, 4, 5] if cfg == "ragged" else None
    _check_against_host(model, emb, k, 12, lengths=lengths)


def test_one_beam_runs_the_beam_kernels(dev):
    """num_beams=1 with return_scores=True takes the beam path with one beam (top 2 per row, the k = 1 bookkeeping)."""
    model = _model(dev)
    emb = _emb(model, 3, 6, seed=2)
    out, sc, lens = _check_against_host(model, emb, 1, 12)
    assert out.shape[0] == 3 and sc.shape == (3,)


# the fp32 oracle on bf16-representable parameters (the engine's own weights), lm_head x 40 so that the beam decisions are
# well separated.  A search over seeds 0..7 at k = 2 picked seed 0: every value a decision compares differs from its neighbour
# by >= ORACLE_MARGIN, while the scores of an eager bf16 run of the oracle moved by at most 0.034
ORACLE_SEED, ORACLE_MARGIN = 0, 0.08


def test_engine_beam_equals_fp32_oracle(dev):
    from magma_amd.sampling import beam_margin, beam_search, reorder_past
    from oracle.model import OracleConfig, init_params, lm_forward
    cfg = OracleConfig.tiny()
    p = init_params(cfg, seed=ORACLE_SEED)
    for key in p:
        if ".adapter." in key:
            p[key] = p[key] * 20
    p["lm.lm_head.weight"] = p["lm.lm_head.weight"] * 40
    p["lm.lm_head.bias"] = p["lm.lm_head.bias"].clone()
    p["lm.lm_head.bias"][cfg.eos_token] += 6.0
    p = {key: (v.to(BF16).float() if v.is_floating_point() else v) for key, v in p.items()}
    lm = {key: v for key, v in p.items() if key.startswith("lm.")}
    B, k, n = 2, 2, 4
    emb = torch.randn(B, 6, cfg.d_model, generator=torch.Generator().manual_seed(ORACLE_SEED)).to(BF16).float()
    box, rec = {}, []

    def step(rows, tokens):
        if rows is None:
            r = lm_forward(lm, cfg, inputs_embeds=emb.repeat_interleave(k, 0))
        else:
            r = lm_forward(lm, cfg, input_ids=tokens[:, None], past=reorder_past(box["past"], rows))
        box["past"] = r["past_key_values"]
        return r["logits"][:, -1].float()

    with torch.no_grad():
        ref_seq, ref_sc, _ = beam_search(step, B, k, n, cfg.eos_token, 1.0, False, k, record=rec)
    margin = beam_margin(rec)
    assert margin >= ORACLE_MARGIN, f"fixture lost its decision margin on this host: {margin}"
    from magma_amd.testing import build_reduced_magma
    model = build_reduced_magma(dev)
    missing, unexpected = model.load_checkpoint_state(p)
    assert not unexpected and not any(key.startswith("lm.") for key in missing), (missing, unexpected)
    model.eval()
    assert model.eos_token == cfg.eos_token
    out, sc = model.generate(emb.to(BF16).to(dev), max_steps=n, num_beams=k, num_return_sequences=k, decode=False,
                             return_scores=True)
    assert torch.equal(out[:, emb.shape[1]:].cpu(), ref_seq), (out, ref_seq)
    assert float((sc - ref_sc).abs().max()) < margin / 2


def test_options_and_rescoring(dev):
    """length_penalty / early_stopping / num_return_sequences through the engine, and every returned hypothesis re-scored by
    the cache-less full-sequence forward: sum of its tokens' log-probabilities == the returned score x len^lp (a wrong or
    missing KV reorder fails this whatever the ranking)."""
    model = _model(dev)
    emb = _emb(model, 2, 6, seed=5)
    for lp, es, n_ret in [(1.0, True, 2), (0.0, "never", 4), (2.0, False, 1), (-0.5, False, 3)]:
        out, sc, lens = _check_against_host(model, emb, 4, 10, lp=lp, es=es, n_ret=n_ret)
        S = emb.shape[1]
        for i in range(out.shape[0]):
            n = int(lens[i])
            toks = out[i, S:S + n]
            e = emb[i // n_ret]
            if n > 1:
                e = torch.cat([e, model.lm.engine.embed_ids(toks[None, :-1])[0]], 0)
            lg = model.lm(inputs_embeds=e[None]).logits[0, S - 1:].float()
            s = float(torch.log_softmax(lg, -1).gather(1, toks[:, None]).sum())
            assert abs(s - float(sc[i]) * n ** lp) <= 0.05 * n, (i, s, float(sc[i]) * n ** lp)   # bf16 logits: ~1e-2 per token


def test_graph_equals_eager_and_sample_alone(dev, monkeypatch):
    model = _model(dev)
    emb = _emb(model, 3, 6, seed=9)
    a, sa = model.generate(emb, max_steps=10, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
    b, sb = model.generate(emb, max_steps=10, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)          # second call replays the captured step
    eng = model.lm.engine
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))
    c, sc = model.generate(emb, max_steps=10, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
    monkeypatch.undo()
    assert torch.equal(a, c) and torch.equal(sa, sc)
    for i in range(3):
        o, s = model.generate(emb[i:i + 1], max_steps=10, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
        assert torch.equal(o, a[2 * i: 2 * i + 2, : o.shape[1]]) and bool((a[2 * i: 2 * i + 2, o.shape[1]:] == model.eos_token).all())
        assert torch.allclose(s, sa[2 * i: 2 * i + 2], rtol=1e-5, atol=1e-5)


def test_decode_true_and_errors(dev):
    model = _model(dev)
    emb = _emb(model, 2, 6, seed=3)
    txt = model.generate(emb, max_steps=6, num_beams=3, num_return_sequences=3)
    assert isinstance(txt, list) and len(txt) == 6 and all(isinstance(t, str) for t in txt)
    for kw in [dict(num_beams=2, num_return_sequences=3), dict(num_beams=0), dict(num_beams=17)]:
        with pytest.raises(ValueError):
            model.generate(emb, max_steps=4, **kw)


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block, B = 2, k = 4: the full-width selection inside the captured step."""
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    emb = _emb(model, 2, 5, seed=4)
    _check_against_host(model, emb, 4, 6)
