"""Diverse beam search on the device (DESIGN.md "Diverse beam search"): the selection kernel at the list lengths k + k / G, the
grouped bookkeeping launch (mg_beam_finish_groups) against the host statement magma_amd.sampling.group_beam_search step for
step, against mg_beam_finish at one group, and generate(num_beam_groups=...) on the reduced model against the host statement
driven by the engine's own decode logits."""
import itertools

import pytest
import torch

import group_beam_cases as GC

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------ the selection kernel
@pytest.mark.parametrize("V", [1056, 50258])
@pytest.mark.parametrize("K2", [3, 6, 9, 17, 24])
def test_selection_kernel_at_group_list_lengths(dev, V, K2):
    """mg_beam_topk_f32 and mg_beam_topk_scores_f32 at list lengths that are not 2k (odd ones among them)."""
    from magma_amd import ops
    R = 4
    x = GC.gapped_logits(R, V, seed=V + K2)
    g = torch.Generator().manual_seed(K2)
    run = (torch.randn(R, generator=g) * 3 - 5).float()
    run[1] = -1e9                                  # a beam that must not expand: every fp32 score of the row rounds to -1e9
    live = run > -1e8
    ld = V + 7
    xd = torch.zeros(R, ld, device=dev)
    xd[:, :V] = x.to(dev)
    pre = torch.zeros(R, ld, device=dev)
    pre[:, :V] = torch.log_softmax(x, -1).to(dev)
    for normalized, rows, lp in ((False, xd, torch.log_softmax(x.double(), -1)), (True, pre, torch.log_softmax(x, -1).double())):
        cs = torch.zeros(R, K2, device=dev)
        ct = torch.full((R, K2), -1, dtype=torch.int32, device=dev)
        ops.beam_topk(rows[:, :V], run.to(dev), cs, ct, normalized=normalized)
        ref_s, ref_t = torch.topk(lp + run.double()[:, None], K2, dim=-1)
        assert torch.equal(ct.cpu().long()[live], ref_t[live]), normalized
        assert torch.allclose(cs.cpu().double()[live], ref_s[live], rtol=1e-6, atol=0), normalized
        sc32 = run[~live][:, None] + lp[~live].float()
        order = torch.sort(-sc32, dim=-1, stable=True)[1][:, :K2]
        assert bool((cs.cpu()[~live] == -1e9).all()) and torch.equal(ct.cpu()[~live].long(), order), normalized


# --------------------------------------------------------------------------------------------------- the bookkeeping launch
def _state(dev, B, k, G, ld, eos=0):
    R = B * k
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    run = z(R, dt=f32)
    run.view(B * G, k // G)[:, 1:] = -1e9
    return dict(run=run, fin_score=torch.full((R,), -1e9, device=dev), fin_flag=z(R, dt=i32), fin_len=z(R, dt=i32),
                fin_tok=torch.full((R, ld), eos, dtype=i64, device=dev), fin_stage=z(R, ld, dt=i64), hist=z(R, ld, dt=i64),
                hist_stage=z(R, ld, dt=i64), unsat=torch.ones(B * G, dtype=i32, device=dev), parent=z(R, dt=i32), token=z(R, dt=i64))


def _round_robin(t, B, k, G):
    """Device slots (sample, group, rank) in the order the host statement returns them: (sample, rank, group)."""
    return t.view(B, G, k // G, *t.shape[1:]).transpose(1, 2).reshape(B * k, *t.shape[1:])


_KG = [(2, 2), (4, 2), (6, 3), (16, 2), (16, 16)]
_LAM = [0.0, 0.5, 1e4]
_RULES = list(itertools.product((1.0, -0.5), (True, False, "never"), ("random", "heavy")))
# the product has 180 members; every (k, G, lambda) keeps 4 of the 12 (length_penalty, early_stopping, eos mode) settings -- a
# third of them, shifted with (k, G) and with lambda, so that every setting meets every (k, G) and every lambda: 60 cases
CASES = [(k, G, lam, lp, es, mode) for a, (k, G) in enumerate(_KG) for b, lam in enumerate(_LAM)
         for j, (lp, es, mode) in enumerate(_RULES) if (a + b + j) % 3 == 0]


def test_cases_cover_the_grid():
    assert len(CASES) == 60
    for col, values in ((3, (1.0, -0.5)), (4, (True, False, "never")), (5, ("random", "heavy"))):
        for kg, lam in itertools.product(_KG, _LAM):
            assert {c[col] for c in CASES if c[:2] == kg} == set(values)
            assert {c[col] for c in CASES if c[2] == lam} == set(values)


@pytest.mark.parametrize("k,G,lam,lp,es,eos_mode", CASES)
def test_bookkeeping_against_host_rule(dev, k, G, lam, lp, es, eos_mode):
    """The selection launch at K2 = k + k' and the grouped bookkeeping launch against the host statement step for step on
    scripted logits; then two more steps past the recorded stop must leave every finished slot as it is.  At lambda = 1e4 all
    rows of a sample hold the same logits at step 0, so group G-1's top 2k' are the ranks [k - k', k + k') of its row: the last
    of them is the last entry of the row's list of k + k', and lies outside a list of 2k' -- asserted from the host record."""
    from magma_amd import ops
    B, V, n, eos = 3, 64, 10, 5
    R, kq = B * k, k // G
    K2 = k + kq
    table, (ref_seq, ref_sc, ref_len), host_parents, rec = GC.scripted_run(k, G, lam, lp, es, eos_mode, B, V, n, eos,
                                                                           same_first=lam == 1e4)
    if lam == 1e4:
        last = rec[G - 1]
        assert last["group"] == G - 1 and last["step"] == 0
        assert int(last["row_rank"].max()) == K2 - 1 >= 2 * kq and bool((last["row_rank"].max(-1).values == K2 - 1).all())
    st = _state(dev, B, k, G, ld=n + 4, eos=eos)
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    cs = torch.zeros(R, K2, device=dev)
    ct = torch.zeros(R, K2, dtype=torch.int32, device=dev)
    dev_parents = []
    for t in range(n):
        ops.beam_topk(table[t].to(dev), st["run"], cs, ct)
        ops.beam_finish_groups(cs, ct, B, k, G, lam, V, eos, lp, es, n, state, st)
        dev_parents.append(st["parent"].cpu().long())
        if int(state[1]) >= 0:
            break
    assert int(state[1]) == len(host_parents), (int(state[1]), len(host_parents))
    for a, b in zip(host_parents, dev_parents):
        assert torch.equal(a, b)
    lens = _round_robin(st["fin_len"].cpu().long(), B, k, G)
    m = int(lens.max())
    assert torch.equal(lens, ref_len) and m == ref_seq.shape[1]
    assert torch.equal(_round_robin(st["fin_tok"].cpu(), B, k, G)[:, :m], ref_seq)
    assert torch.allclose(_round_robin(st["fin_score"].cpu(), B, k, G), ref_sc, rtol=1e-6, atol=1e-6)
    assert bool(st["fin_flag"].bool().all())
    frozen = {name: st[name].clone() for name in ("fin_score", "fin_flag", "fin_len", "fin_tok", "unsat")}
    stop, t0 = int(state[1]), int(state[0])
    for t in range(t0, min(t0 + 2, n)):
        ops.beam_topk(table[t].to(dev), st["run"], cs, ct)
        ops.beam_finish_groups(cs, ct, B, k, G, lam, V, eos, lp, es, n, state, st)
        assert torch.equal(st["parent"].cpu(), torch.arange(R, dtype=torch.int32))
    assert int(state[1]) == stop and all(torch.equal(frozen[name], st[name]) for name in frozen)


@pytest.mark.parametrize("k", [1, 4])
def test_one_group_is_the_plain_launch(dev, k):
    """mg_beam_finish_groups(G = 1, lambda = 0, K2 = 2k) writes what mg_beam_finish writes, bit for bit, over 10 steps."""
    from magma_amd import ops
    B, V, n, eos = 3, 64, 10, 5
    R = B * k
    table = GC.scripted(k, 1.0, False, "random", B, V, n, eos)
    a, b = _state(dev, B, k, 1, ld=n + 4, eos=eos), _state(dev, B, k, 1, ld=n + 4, eos=eos)
    sa, sb = (torch.tensor([0, -1], dtype=torch.int32, device=dev) for _ in range(2))
    cs = torch.zeros(R, 2 * k, device=dev)
    ct = torch.zeros(R, 2 * k, dtype=torch.int32, device=dev)
    finished = False
    for t in range(n):
        ops.beam_topk(table[t].to(dev), a["run"], cs, ct)
        ops.beam_finish(cs, ct, B, k, V, eos, 1.0, False, n, sa, a)
        ops.beam_topk(table[t].to(dev), b["run"], cs, ct)
        ops.beam_finish_groups(cs, ct, B, k, 1, 0.0, V, eos, 1.0, False, n, sb, b)
        assert torch.equal(sa, sb)
        for name in a:
            assert torch.equal(a[name], b[name]), (t, name)
        finished = finished or bool(a["fin_flag"].any())
    assert finished and int(sa[0]) == n


def test_launch_validation(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    B, k, V = 1, 4, 64
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    for G, K2, lam in [(2, 8, 0.5), (2, 5, 0.5), (1, 6, 0.0), (2, 6, -1.0), (2, 6, float("inf")), (2, 6, float("nan"))]:
        cs = torch.zeros(B * k, K2, device=dev)
        ct = torch.zeros(B * k, K2, dtype=torch.int32, device=dev)
        with pytest.raises(MagmaHipError):
            ops.beam_finish_groups(cs, ct, B, k, G, lam, V, 5, 1.0, False, 4, state, _state(dev, B, k, G, ld=8))
    with pytest.raises(ValueError):
        ops.beam_finish_groups(cs, ct, B, k, 3, 0.0, V, 5, 1.0, False, 4, state, _state(dev, B, k, 1, ld=8))


# ------------------------------------------------------------------------------------------------------- the reduced model
def _model(dev, **kw):
    from magma_amd.testing import build_reduced_magma
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


def _host_on_engine(model, emb, k, G, lam, n, n_ret, lengths=None, processors=None):
    """The host statement driven by the engine's own cached decode: cache rows reordered by index_select, greedy step, the
    logits of every row -- the same kernels, so the same logits for the same cache contents."""
    from magma_amd.sampling import check_processor_args, group_beam_search
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

    proc = None if processors is None else check_processor_args(**processors)
    return group_beam_search(step, emb.shape[0], k, G, lam, n, model.eos_token, 1.0, False, n_ret, processors=proc)


def _check_against_host(model, emb, k, G, lam, n, n_ret=None, lengths=None, processors=None):
    n_ret = n_ret or k
    ref_seq, ref_sc, ref_len = _host_on_engine(model, emb, k, G, lam, n, n_ret, lengths, processors)
    out, sc = model.generate(emb, max_steps=n, num_beams=k, num_beam_groups=G, diversity_penalty=lam, num_return_sequences=n_ret,
                             decode=False, return_scores=True, lengths=lengths, **(processors or {}))
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


@pytest.mark.parametrize("cfg", ["v1", "ragged", "processors", "wide", "three_groups"])
def test_engine_equals_host_statement(dev, cfg):
    model = _model(dev)
    B = 5 if cfg == "wide" else 3                  # wide: 20 rows, the eager tile-GEMM step
    k, G, n_ret = (6, 3, 3) if cfg == "three_groups" else (4, 2, None)
    emb = _emb(model, B, 7, seed=40 + len(cfg))
    _check_against_host(model, emb, k, G, 0.5, 8, n_ret=n_ret, lengths=[7, 4, 5] if cfg == "ragged" else None,
                        processors=dict(repetition_penalty=1.3, no_repeat_ngram_size=2) if cfg == "processors" else None)


def test_defaults_unchanged(dev):
    from magma_amd.engine import LMEngine
    model = _model(dev)
    emb = _emb(model, 2, 6, seed=1)
    kw = dict(max_steps=8, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
    a, sa = model.generate(emb, **kw)
    b, sb = model.generate(emb, **kw, num_beam_groups=1, diversity_penalty=0.0)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    plain = LMEngine.selection_plan(beam=(4, 1.0, False, 8), vocab=model.lm.engine.V)
    one = LMEngine.selection_plan(beam=(4, 1.0, False, 8, 1, 0.0), vocab=model.lm.engine.V)
    two = LMEngine.selection_plan(beam=(4, 1.0, False, 8, 2, 0.5), vocab=model.lm.engine.V)
    assert plain.mode == one.mode == ("beam", 4, 1.0, False, 8) and plain.keys == one.keys
    assert two.mode == ("beam", 4, 1.0, False, 8, 2, 0.5) and two.keys != plain.keys
    assert two.keys != LMEngine.selection_plan(beam=(4, 1.0, False, 8, 2, 0.25), vocab=model.lm.engine.V).keys


def test_graph_equals_eager_and_sample_alone(dev, monkeypatch):
    model = _model(dev)
    emb = _emb(model, 3, 6, seed=9)
    kw = dict(max_steps=10, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, num_return_sequences=2, decode=False,
              return_scores=True)
    a, sa = model.generate(emb, **kw)
    b, sb = model.generate(emb, **kw)
    assert torch.equal(a, b) and torch.equal(sa, sb)          # second call replays the captured step
    eng = model.lm.engine
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **k2: orig(*x, **{**k2, "use_graph": False}))
    c, sc = model.generate(emb, **kw)
    monkeypatch.undo()
    assert torch.equal(a, c) and torch.equal(sa, sc)
    for i in range(3):
        o, s = model.generate(emb[i:i + 1], **kw)
        assert torch.equal(o, a[2 * i: 2 * i + 2, : o.shape[1]]) and bool((a[2 * i: 2 * i + 2, o.shape[1]:] == model.eos_token).all())
        assert torch.allclose(s, sa[2 * i: 2 * i + 2], rtol=1e-5, atol=1e-5)
    # plain beam search on the same cache afterwards: the buffers are re-armed for one group
    p, sp = model.generate(emb, max_steps=10, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
    q, sq = _model(dev).generate(emb, max_steps=10, num_beams=4, num_return_sequences=2, decode=False, return_scores=True)
    assert torch.equal(p, q) and torch.equal(sp, sq)


def test_it_is_diverse(dev):
    """Four groups of one beam under a penalty that dominates: the four hypotheses of a sample start with four different tokens
    (eos is banned at the first step, so every group's one lineage starts with the token it selected there).  At penalty 0
    the four groups are the same search."""
    model = _model(dev)
    emb = _emb(model, 2, 6, seed=6)
    kw = dict(max_steps=8, num_beams=4, num_beam_groups=4, num_return_sequences=4, decode=False, return_scores=True, min_new_tokens=1)
    out, _ = model.generate(emb, diversity_penalty=1e4, **kw)
    first = out[:, emb.shape[1]].view(2, 4).cpu()
    for row in first:
        assert len(set(row.tolist())) == 4, first
    same, sc = model.generate(emb, diversity_penalty=0.0, **kw)
    same = same.view(2, 4, -1)
    assert all(torch.equal(same[:, 0], same[:, g]) for g in range(1, 4))
    assert torch.allclose(sc.view(2, 4), sc.view(2, 4)[:, :1].expand(2, 4), rtol=1e-5, atol=1e-5)


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block, B = 2, k = 4 in two groups: the full-width selection at K2 = 6 inside the captured step."""
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    emb = _emb(model, 2, 5, seed=4)
    _check_against_host(model, emb, 4, 2, 0.5, 6)
