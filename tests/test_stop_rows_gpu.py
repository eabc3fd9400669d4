"""Per-row stopping on the device (DESIGN.md "Per-row stopping"): the bookkeeping kernel (ops.sample_finish_rows) against the host
statement (magma_amd.sampling.stop_update, pinned to transformers by tests/test_stop_rows_cpu.py) on crafted token scripts --
token, history, finish record, state and d_pos equal at every step --, the extended min-new-tokens rule of ops.logits_process,
and generate(eos_token=[...], stop_sequences=..., stop_per_row=..., return_finish=...) on the reduced model against the host
rule driven by the engine's own decode logits."""
import pytest
import torch

from test_beam_search_gpu import _emb, _model
from test_logits_processors_gpu import _bits, _kernel_inputs, _rows
from test_stop_rows_cpu import _outcome, _stops_from

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------- the kernel
PAD = 40
EOS8 = [PAD, 41, 42, 43, 44, 45, 46, 47]
S1, S2, S16 = [50], [51, 52], list(range(60, 76))
SEQS = [S16,                    # 0
        S2,                     # 1
        S1,                     # 2
        [80, 81, 82],           # 3: [81, 82] (5) is a suffix of it -- the lower index is reported
        [90, 44],               # 4: ends in an eos id -- eos wins
        [81, 82],               # 5
        [85, 86],               # 6: a suffix of 7, and the lower index
        [84, 85, 86],           # 7
        [PAD, PAD],             # 8: the padded tail of a finished row
        [52, PAD],              # 9: the end of a stop sequence, then the pad
        [91], [92], [93], [94], [95], [96, 97]]
FILL = 7                        # in no item


def _templates(cols):
    """(script of `cols` tokens, step at which the row finishes or None, reason code or None): sequence lengths 1, 2 and 16
    ending at steps L - 1 (the first step that can match) and L, their last L - 1 tokens ending at step L - 2 (cannot match),
    a length-1 sequence and an eos id at step 0, suffixes, eos against a sequence, and padded tails that would match."""
    from magma_amd.ops import STOP_EOS, STOP_SEQ
    rows = []

    def add(head, step, code):
        rows.append((head + [FILL] * (cols - len(head)), step, code))

    for j, q in ((2, S1), (1, S2), (0, S16)):
        add(q, len(q) - 1, STOP_SEQ | j)
        add([FILL] + q, len(q), STOP_SEQ | j)
    add([43], 0, STOP_EOS | 3)
    add([FILL, FILL, 47], 2, STOP_EOS | 7)
    add([80, 81, 82], 2, STOP_SEQ | 3)
    add([FILL, 81, 82], 2, STOP_SEQ | 5)
    add([84, 85, 86], 2, STOP_SEQ | 6)
    add([90, 44], 1, STOP_EOS | 4)
    add([FILL, PAD, PAD, PAD], 1, STOP_EOS | 0)         # the pad id itself: eos 0, then a tail [PAD, PAD] that would match 8
    add([51, 52, PAD], 1, STOP_SEQ | 1)                # finished by sequence 1; [52, PAD] (9) would match one step later
    add([96, 96, 97], 2, STOP_SEQ | 15)
    n_finishing = len(rows)
    add(S2[1:], None, None)                            # the last L - 1 tokens at step L - 2
    add(S16[1:], None, None)
    add([FILL] * cols, None, None)
    add([52, 51, 82, 81, 97, 96], None, None)          # every item's tokens, never in order
    return rows, n_finishing


def _host_step(tok, hist, cols, step, fin, state, d_pos, delta, eos_ids, seqs):
    """One launch, on the host: stop_update is the rule, the rest is the bookkeeping of mg_sample_finish."""
    from magma_amd.sampling import stop_update
    done = fin[:, 0] >= 0
    tok[done] = eos_ids[0]
    if step < cols:
        hist[:, step] = tok
        now, why = stop_update(hist, step, done, eos_ids, seqs)
    else:                                   # past the history: nothing is recorded, no sequence can be matched
        now, why = stop_update(tok[:, None], 0, done, eos_ids, ())
    new = now & ~done
    fin[new, 0] = step
    fin[new, 1] = (why[new, 0] * 256 + why[new, 1]).to(fin.dtype)
    if bool(now.all()) and int(state[1]) < 0:
        state[1] = step
    state[0] = step + 1
    d_pos += delta


@pytest.mark.parametrize("per_row_pos", [False, True], ids=["uniform", "per_row"])
@pytest.mark.parametrize("B,all_finish", [(1, True), (5, True), (5, False), (300, True), (300, False)])
def test_kernel_equals_host_statement_at_every_step(dev, B, all_finish, per_row_pos):
    from magma_amd import ops
    cols, n_steps, delta = 20, 23, 1
    rows, n_fin = _templates(cols)
    pick = rows[:n_fin] if all_finish else rows
    if B == 1:
        pick = [rows[1]]                    # [FILL, 50]: finishes at step 1
    elif B == 5:
        pick = [rows[5], rows[3], rows[12], rows[13], rows[7]] if all_finish else [rows[5], rows[n_fin], rows[12], rows[13], rows[-1]]
    script = torch.tensor([pick[(b * 7) % len(pick) if B > 5 else b][0] + [FILL, 41, FILL] for b in range(B)], dtype=torch.int64)
    want = [pick[(b * 7) % len(pick) if B > 5 else b][1:] for b in range(B)]
    if not all_finish:                      # unfinished rows meet eos id 1 at step cols + 1, past the history
        want = [w if w[0] is not None else (cols + 1, ops.STOP_EOS | 1) for w in want]
    table = ops.stop_table(EOS8, SEQS).to(dev)
    # every buffer inside a larger one filled with a sentinel
    big_h = torch.full((B + 2, cols + 9), -77, dtype=torch.int64, device=dev)
    big_f = torch.full((B + 2, 2), -77, dtype=torch.int32, device=dev)
    big_t = torch.full((B + 2,), -77, dtype=torch.int64, device=dev)
    big_p = torch.full(((B if per_row_pos else 1) + 2,), -77, dtype=torch.int32, device=dev)
    hist_d, fin_d, tok_d, pos_d = big_h[1:B + 1, 4:4 + cols], big_f[1:B + 1], big_t[1:B + 1], big_p[1:-1]
    hist_d.fill_(-5)
    fin_d.copy_(torch.tensor([[-1, 0]] * B, dtype=torch.int32))
    pos_d.copy_(torch.arange(pos_d.numel(), dtype=torch.int32) * 3 + 11)
    state_d = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    hist = torch.full((B, cols), -5, dtype=torch.int64)
    fin = torch.tensor([[-1, 0]] * B, dtype=torch.int64)
    state, pos = torch.tensor([0, -1]), torch.arange(pos_d.numel()) * 3 + 11
    first_all = []
    for step in range(n_steps):
        tok = script[:, step].clone()
        tok_d.copy_(tok)
        ops.sample_finish_rows(tok_d, state_d, table, len(EOS8), len(SEQS), PAD, fin_d, d_pos=pos_d, delta=delta, history=hist_d,
                               pos_stride=1 if per_row_pos else 0)
        _host_step(tok, hist, cols, step, fin, state, pos, delta, EOS8, SEQS)
        assert torch.equal(tok_d.cpu(), tok), (step, tok_d.cpu(), tok)
        assert torch.equal(hist_d.cpu(), hist), step
        assert torch.equal(fin_d.cpu().to(torch.int64), fin), (step, fin_d.cpu(), fin)
        assert state_d.tolist() == state.tolist() and pos_d.tolist() == pos.tolist(), (step, state_d, state)
        if int(state[1]) >= 0 and not first_all:
            first_all.append(step)
    # the rule did what the script was written for: every row's step and reason, the padded rows never looked at again
    assert [tuple(f) for f in fin.tolist()] == [tuple(w) for w in want]
    last = max(w[0] for w in want)
    assert first_all == [last] and int(state[1]) == last        # written once, at the step the last row finished
    assert last == (cols + 1 if not all_finish else 1 if B == 1 else 16)      # the last row finishes late, or past the history
    # sentinels
    inner = torch.zeros_like(big_h, dtype=torch.bool)
    inner[1:B + 1, 4:4 + cols] = True
    assert bool((big_h[~inner] == -77).all())
    assert bool((big_f[0] == -77).all()) and bool((big_f[-1] == -77).all())
    assert big_t[0] == -77 and big_t[-1] == -77 and big_p[0] == -77 and big_p[-1] == -77


def test_kernel_one_eos_no_row_finished_is_sample_finish(dev):
    """n_seq = 0, one eos id and no row finished: every output is ops.sample_finish's -- history, state, d_pos, the cleared
    counters, the token untouched -- on uniform and per-row positions, with and without a history."""
    from magma_amd import ops
    B, cols = 37, 6
    g = torch.Generator().manual_seed(3)
    table = ops.stop_table([PAD]).to(dev)
    for ps in (0, 1):
        for with_hist in (True, False):
            outs = []
            for rows in (False, True):
                tok = torch.randint(100, 200, (B,), generator=g.manual_seed(9)).to(dev)
                state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
                pos = torch.full((B if ps else 1,), 13, dtype=torch.int32, device=dev)
                hist = torch.full((B, cols + 3), -5, dtype=torch.int64, device=dev)
                clear = torch.full((4 * 16,), 9, dtype=torch.int32, device=dev)
                fin = torch.tensor([[-1, 0]] * B, dtype=torch.int32, device=dev)
                for step in range(cols + 2):
                    tok.add_(1)
                    kw = dict(d_pos=pos, delta=2, history=hist[:, :cols] if with_hist else None, clear=clear, clear_stride=16, pos_stride=ps)
                    if rows:
                        ops.sample_finish_rows(tok, state, table, 1, 0, PAD, fin, **kw)
                    else:
                        ops.sample_finish(tok, PAD, state, **kw)
                assert bool((fin.cpu() == torch.tensor([-1, 0], dtype=torch.int32)).all())
                outs.append([t.cpu() for t in (tok, state, pos, hist, clear)])
            assert all(torch.equal(a, b) for a, b in zip(*outs)), (ps, with_hist)
            assert outs[0][1].tolist() == [cols + 2, -1] and bool((outs[0][4][::16] == 0).all())
    # all rows at the eos id at one step: both record it
    tok = torch.full((B,), PAD, dtype=torch.int64, device=dev)
    s_a, s_b = (torch.tensor([4, -1], dtype=torch.int32, device=dev) for _ in range(2))
    fin = torch.tensor([[-1, 0]] * B, dtype=torch.int32, device=dev)
    ops.sample_finish(tok, PAD, s_a)
    ops.sample_finish_rows(tok, s_b, table, 1, 0, PAD, fin)
    assert s_a.tolist() == s_b.tolist() == [5, 4] and fin.tolist() == [[4, ops.STOP_EOS]] * B


def test_kernel_refusals(dev):
    from magma_amd import ops
    tok = torch.zeros(3, dtype=torch.int64, device=dev)
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    fin = torch.zeros(3, 2, dtype=torch.int32, device=dev)
    table = ops.stop_table([1], [[2, 3]]).to(dev)
    for n_eos, n_seq, hist in ((0, 0, None), (9, 0, None), (1, 17, torch.zeros(3, 4, dtype=torch.int64, device=dev)), (1, -1, None),
                               (1, 1, None)):          # stop sequences without a history to match them against
        with pytest.raises(ops.L.MagmaHipError):
            ops.sample_finish_rows(tok, state, table, n_eos, n_seq, 1, fin, history=hist)
    assert state.tolist() == [0, -1]


@pytest.mark.parametrize("V", [1056, 50258])
def test_min_new_tokens_with_further_eos_ids(dev, V):
    """NULL / 0: the bits of the call without them; two further ids: banned below min_new_tokens, free from it on."""
    from magma_amd import ops
    from magma_amd.sampling import process_logits
    R, eos, more = 3, 3, [V - 1, 17]
    full, hist = _kernel_inputs(R, V, seed=V)
    more_d = torch.tensor(more + [5, 6, 7, 9, 11], dtype=torch.int32, device=dev)      # the ids past n_eos_more do not count
    for step in (0, 3, 4, 9):
        for rules in (dict(min_new_tokens=4), dict(min_new_tokens=4, repetition_penalty=1.3, no_repeat_ngram_size=2)):
            state = torch.tensor([step, -1], dtype=torch.int32, device=dev)
            base = full.to(dev)
            ops.logits_process(base[:, :V], state, hist.to(dev), eos=eos, **rules)
            for kw in (dict(), dict(eos_more=None, n_eos_more=0), dict(eos_more=more_d, n_eos_more=0)):
                x = full.to(dev)
                ops.logits_process(x[:, :V], state, hist.to(dev), eos=eos, **rules, **kw)
                assert torch.equal(_bits(x), _bits(base))
            want = full.clone()
            want[:, :V] = process_logits(full[:, :V], hist, step, eos_token=[eos] + more, **rules)
            assert torch.equal(_bits(base.cpu()), _bits(want)) == (step >= 4)
            x = full.to(dev)
            ops.logits_process(x[:, :V], state, hist.to(dev), eos=eos, eos_more=more_d, n_eos_more=2, **rules)
            assert torch.equal(_bits(x.cpu()), _bits(want)), (step, rules)
            assert bool((x[:, more] == float("-inf")).all()) == (step < 4)


# ------------------------------------------------------------------------------------------------------- the reduced model
N = 12


def _diverse(dev, monkeypatch=None, **kw):
    """The reduced model of tests/test_beam_search_gpu.py with the eos bias that _model adds taken off again: with it every greedy
    row is eos from step 0 on, so no two rows could finish at different steps; without it the rows differ from the first token."""
    model = _model(dev, monkeypatch, **kw)
    with torch.no_grad():
        model.lm.lm_head.bias[model.eos_token] -= 4.0
        model.lm.invalidate_packed()
    return model


def _host_loop(model, emb, n, eos_ids, seqs, rules=None, lengths=None, select=None, past=None, stop_on_eos=True):
    """The host rule driven by the engine's own logits (as _host_loop of test_logits_processors_gpu.py): prefill (or the new rows
    appended to ``past``), then eager decode steps fed the host's choice -- raw logits, host process_logits (every eos id banned
    by min_new_tokens), ``select`` (default argmax), the pad id for a finished row, stop_update.  Returns (tokens (B, width),
    finish record (B, 2) as the device keeps it)."""
    from magma_amd.sampling import process_logits, stop_update
    eng = model.lm.engine
    kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths)}
    o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=n, past_key_values=past, **kw)
    c = o.past_key_values
    lg = o.logits[:, -1].float().cpu()
    B = emb.shape[0]
    hist = torch.zeros(B, n, dtype=torch.int64)
    done, rec = torch.zeros(B, dtype=torch.bool), torch.tensor([[-1, 0]] * B)
    width = n
    for t in range(n):
        x = process_logits(lg, hist, t, eos_token=list(eos_ids), **(rules or {}))
        tok = x.argmax(-1) if select is None else select(x, t)
        hist[:, t] = torch.where(done, torch.full_like(tok, eos_ids[0]), tok)
        now, why = stop_update(hist, t, done, eos_ids, seqs)
        new = now & ~done
        rec[new, 0], rec[new, 1] = t, why[new, 0] * 256 + why[new, 1]
        done = now
        if bool(done.all()) and stop_on_eos:
            width = t + 1
            break
        if t + 1 < n:
            lg = eng.decode(hist[:, t:t + 1].to(model.device), c, use_graph=False)[0].float().cpu()
    return hist[:, :width], rec


def _gen(model, emb, eos_ids, seqs, n=N, lengths=None, **kw):
    kw.setdefault("temperature", 0.0)
    out, fin = model.generate(emb, max_steps=n, decode=False, lengths=lengths, eos_token=list(eos_ids), stop_sequences=seqs,
                              return_finish=True, **kw)
    S = emb.shape[1]
    return _rows(out, S, out.shape[1] - S, lengths), fin


def _plain(model, emb, n=N, lengths=None, **kw):
    kw.setdefault("temperature", 0.0)
    out = model.generate(emb, max_steps=n, decode=False, stop_on_eos=False, lengths=lengths, **kw)
    return _rows(out, emb.shape[1], n, lengths)


def _check(got, fin, ref, rec, leave):
    """Outputs and finish records equal the host loop's; the run exercised the rule: three distinct finishing steps or more,
    both reasons, a row that never finishes exactly when one was left alone (``leave`` "any": either way)."""
    from magma_amd.sampling import finish_from_record
    steps = {int(f) for f, _ in rec.tolist() if f >= 0}
    assert len(steps) >= 3 and {c >> 8 for f, c in rec.tolist() if f >= 0} == {1, 2}, rec
    assert leave == "any" or bool((rec[:, 0] < 0).any()) == (leave is not None), rec
    assert got.shape == ref.shape and torch.equal(got, ref), (got, ref)
    want = finish_from_record(rec, ref.shape[1])
    assert torch.equal(fin.kept, want.kept) and fin.reason == want.reason and fin.index == want.index, (fin, want)
    if not bool((rec[:, 0] < 0).any()):
        assert ref.shape[1] == max(steps) + 1 and (leave == "any" or ref.shape[1] < N)


@pytest.mark.parametrize("cfg", ["v1", "ragged", "wide", "w8", "rules"])
def test_engine_greedy_equals_host_rule(dev, monkeypatch, cfg):
    kw = {"w8": dict(n_layer=1, n_head=16, d_ff=4096)}.get(cfg, {})
    model = _diverse(dev, monkeypatch, w8=cfg == "w8", **kw)
    assert model.lm.engine.decode_w8 == (cfg == "w8")
    B, S = (20 if cfg == "wide" else 5), 7
    emb = _emb(model, B, S, seed=140 + len(cfg))
    lengths = [7, 4, 5, 6, 3] if cfg == "ragged" else None
    leave = 3 if cfg == "ragged" else None
    rules = {}
    if cfg == "rules":        # the four logits processors on: three of them from the plain run's tokens, min_new_tokens below
        first = _plain(model, emb)
        rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=tuple(dict.fromkeys(first[:, 1].tolist()))[:3])
    plain = _plain(model, emb, lengths=lengths, **rules)
    eos_ids, seqs = _stops_from(plain if leave is not None else plain[:, :N - 2], leave)      # (all finished: before the last step)
    if cfg == "rules":        # min_new_tokens above the earliest step at which an eos id of the list finishes a row: it bans them all
        _, rec0 = _host_loop(model, emb, N, eos_ids, seqs, rules)
        first_eos = min(f for f, c in rec0.tolist() if f >= 0 and c >> 8 == 1)
        rules["min_new_tokens"] = first_eos + 1
        assert len(eos_ids) > 1
        leave = "any"
    ref, rec = _host_loop(model, emb, N, eos_ids, seqs, rules, lengths)
    if cfg == "rules":
        assert not torch.equal(rec, rec0), "min_new_tokens left every row finishing as it did"
        assert all(f > first_eos for f, c in rec.tolist() if f >= 0 and c >> 8 == 1), rec
    got, fin = _gen(model, emb, eos_ids, seqs, lengths=lengths, **rules)
    _check(got, fin, ref, rec, leave)
    # stop_on_eos=False: all max_steps, the finished rows padded
    full, fin_full = _gen(model, emb, eos_ids, seqs, lengths=lengths, stop_on_eos=False, **rules)
    ref_full, _ = _host_loop(model, emb, N, eos_ids, seqs, rules, lengths, stop_on_eos=False)
    assert full.shape[1] == N and torch.equal(full, ref_full) and fin_full.reason == fin.reason


def test_engine_sampled_equals_host_rule(dev):
    """Fixed seed: the host loop draws with ops.sample at the same seed and step; a finished row does not disturb the others."""
    from magma_amd import ops
    model = _diverse(dev)
    B, S, seed = 5, 7, 4321
    emb = _emb(model, B, S, seed=160)
    mode = dict(temperature=0.7, top_k=8, top_p=0.9)
    seed_d = torch.tensor([seed], dtype=torch.int64, device=dev)

    def draw(x, t):
        state = torch.tensor([t, -1], dtype=torch.int32, device=dev)
        return ops.sample(x.to(dev), mode["temperature"], mode["top_k"], mode["top_p"], seed_d, state).cpu()

    plain = _plain(model, emb, seed=seed, **mode)
    eos_ids, seqs = _stops_from(plain[:, :N - 2])
    ref, rec = _host_loop(model, emb, N, eos_ids, seqs, select=draw)
    got, fin = _gen(model, emb, eos_ids, seqs, seed=seed, **mode)
    _check(got, fin, ref, rec, None)
    for r in range(B):        # every row up to its finishing token is the plain run's row
        assert torch.equal(got[r, : int(fin.kept[r])], plain[r, : int(fin.kept[r])])


def test_early_exit_and_one_eos_id(dev):
    """stop_on_eos=True returns after the step at which the last row finished, and the device ran at most eos_check_every steps
    more; stop_per_row=True with the model's one eos id gives the plain batch the same early exit."""
    model = _diverse(dev)
    B, S, n, every = 5, 7, 32, 4
    emb = _emb(model, B, S, seed=141)
    eos_ids, seqs = _stops_from(_plain(model, emb, n=N))
    out, past, fin = model.generate(emb, max_steps=n, temperature=0.0, decode=False, eos_token=eos_ids, stop_sequences=seqs,
                                    eos_check_every=every, return_past_key_values=True, return_finish=True)
    last = int(fin.kept.max()) - 1
    assert "length" not in fin.reason and out.shape[1] == S + last + 1 < S + n
    assert last + 1 <= int(past.sample_state[0]) <= last + 1 + every and int(past.sample_state[1]) == last
    # one eos id, the model's, on _model itself (eos favoured) and sampled, so that the rows reach it at different steps: the
    # plain run's rows, each cut at its own first eos
    model = _model(dev)
    eos = model.eos_token
    mode = dict(temperature=1.0, top_k=8, seed=4321)
    plain = _plain(model, emb, n=n, **mode)
    at = [r.tolist().index(eos) if eos in r.tolist() else None for r in plain]
    assert all(a is not None for a in at) and len(set(at)) > 1, at
    out, fin = model.generate(emb, max_steps=n, decode=False, stop_per_row=True, return_finish=True, **mode)
    assert out.shape[1] == S + max(at) + 1 and fin.kept.tolist() == [a + 1 for a in at] and fin.reason == ["eos"] * B
    for r in range(B):
        assert torch.equal(out[r, S:S + at[r] + 1].cpu(), plain[r, :at[r] + 1]) and bool((out[r, S + at[r]:] == eos).all())
    old = model.generate(emb, max_steps=n, decode=False, **mode)      # the reference's rule: a step at which EVERY row selects eos
    assert old.shape[1] >= out.shape[1]


def test_default_path_keeps_its_bits_and_launches(dev, monkeypatch):
    """Today's arguments: the host loop's ids, the launches of a call before any per-row call on the cache -- mg_sample_finish
    among them, the per-row launch not -- also after per-row calls used the same cache; a per-row call swaps exactly that launch."""
    from launch_trace import record
    from magma_amd import ops
    from test_logits_processors_gpu import _host_loop as plain_host_loop
    model = _diverse(dev)
    eng = model.lm.engine
    B, S = 3, 7
    emb = _emb(model, B, S, seed=142)
    calls = {"rows": 0, "plain": 0}
    real_rows = ops.sample_finish_rows
    monkeypatch.setattr(ops, "sample_finish_rows", lambda *a, **kw: (calls.__setitem__("rows", calls["rows"] + 1), real_rows(*a, **kw))[1])
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))

    def default(**kw):
        return model.generate(emb, max_steps=5, temperature=0.0, decode=False, stop_on_eos=False, **kw)

    rec_a, out_a = record(eng, default)
    assert not isinstance(out_a, Exception), out_a
    assert torch.equal(out_a[:, S:].cpu(), plain_host_loop(model, emb, 5, {}))
    assert calls["rows"] == 0 and sum(r["op"] == "sample_finish" for r in rec_a) == 5
    plain = out_a[:, S:].cpu()
    eos_ids, seqs = [int(plain[0, 1]), int(plain[1, 0])], [plain[2, 1:3].tolist()]
    rec_s, out_s = record(eng, lambda: default(eos_token=eos_ids, stop_sequences=seqs))
    assert not isinstance(out_s, Exception), out_s
    assert calls["rows"] == 5 and [r["op"] for r in rec_s] == [r["op"] for r in rec_a if r["op"] != "sample_finish"]
    for extra in (dict(), dict(stop_per_row=None, stop_sequences=None, eos_token=None, return_finish=False), dict(stop_per_row=False)):
        rec_b, out_b = record(eng, lambda: default(**extra))
        assert not isinstance(out_b, Exception), out_b
        assert torch.equal(out_a, out_b) and rec_a == rec_b
    assert calls["rows"] == 5


def test_graph_replay_new_table_new_counts_and_eager(dev, monkeypatch):
    model = _diverse(dev)
    eng = model.lm.engine
    B, S = 5, 7
    emb = _emb(model, B, S, seed=143)
    plain = _plain(model, emb)
    eos_ids, seqs = _stops_from(plain[:, :N - 2])
    ref, rec = _host_loop(model, emb, N, eos_ids, seqs)
    a, _ = _gen(model, emb, eos_ids, seqs)          # eager first step, captures the second, replays the rest
    b, _ = _gen(model, emb, eos_ids, seqs)          # replays every step
    assert torch.equal(a, ref) and torch.equal(b, ref)
    graphs = next(iter(eng._cache_pool.values())).decode_state.graphs
    n_graphs = len(graphs)
    # the same counts, other items: the captured step is replayed and obeys the new table
    rows = plain.tolist()
    eos2 = [eos_ids[0]] + [rows[r % B][2 + r] for r in range(1, len(eos_ids))]
    seqs2 = [rows[(j + 2) % B][3 + j: 3 + j + len(q)] for j, q in enumerate(seqs)]
    assert (eos2, seqs2) != (eos_ids, seqs) and [len(q) for q in seqs2] == [len(q) for q in seqs]
    ref2, rec2 = _host_loop(model, emb, N, eos2, seqs2)
    assert not torch.equal(rec2, rec), "the second table finishes the rows as the first"
    got2, fin2 = _gen(model, emb, eos2, seqs2)
    assert torch.equal(got2, ref2) and len(graphs) == n_graphs
    # other counts: a step captured under its own key
    eos3, seqs3 = eos_ids + [rows[0][-1]], seqs[:-1]
    ref3, _ = _host_loop(model, emb, N, eos3, seqs3)
    got3, _ = _gen(model, emb, eos3, seqs3)
    assert torch.equal(got3, ref3) and len(graphs) == n_graphs + 1
    # the eager step agrees with the captured one
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))
    e, _ = _gen(model, emb, eos_ids, seqs)
    assert torch.equal(e, ref)
    monkeypatch.undo()
    assert torch.equal(_plain(model, emb), plain)


def test_multi_turn_keeps_stop_text_and_cuts_eos(dev):
    """A row stopped by a sequence, a row stopped by an eos id and an unfinished row, continued: the ids of a fresh call over
    [prompt ; kept tokens ; new input] -- the stop text kept, the eos dropped (tied candidates aside, as in
    tests/test_continue_generate_gpu.py)."""
    from test_continue_generate_gpu import agree, embeds, new_tokens
    model = _diverse(dev)
    wte = model.lm.engine.wte
    never = -7
    prompts, q = embeds(model, [9, 5, 7], seed=144), embeds(model, [3, 6, 2], seed=145)
    lens = [p.shape[0] for p in prompts]
    plain = torch.tensor(new_tokens(model.generate(prompts, max_steps=N, temperature=0.0, decode=False, stop_on_eos=False), lens, never, N))
    rows = plain.tolist()
    found = [(a, b) for a in range(1, N - 1) for b in range(1, N - 1)
             if _outcome(rows, [rows[0][a]], [rows[1][b - 1: b + 1]]) == [(a, "eos"), (b, "stop"), None]]
    assert found, f"no eos id of row 0 and sequence of row 1 that leave row 2 alone: {rows}"
    t0, t1 = found[0]
    eos_ids, seqs = [rows[0][t0]], [rows[1][t1 - 1: t1 + 1]]
    out, past, fin = model.generate(prompts, max_steps=N, temperature=0.0, decode=False, eos_token=eos_ids, stop_sequences=seqs,
                                    return_past_key_values=True, return_finish=True)
    assert fin.reason == ["eos", "stop", "length"] and fin.kept.tolist() == [t0 + 1, t1 + 1, N] and fin.index == [0, 0, -1]
    assert torch.equal(out[1, lens[1]: lens[1] + t1 + 1].cpu(), plain[1, : t1 + 1])
    keep = [rows[0][:t0], rows[1][: t1 + 1], rows[2]]
    conv = [torch.cat([p, wte[torch.tensor(k, dtype=torch.long, device=p.device)], x], 0) for p, k, x in zip(prompts, keep, q)]
    got = model.generate(q, max_steps=6, temperature=0.0, decode=False, stop_on_eos=False, past_key_values=past)
    fresh = model.generate(conv, max_steps=6, temperature=0.0, decode=False, stop_on_eos=False)
    agree(model, conv, new_tokens(got, [x.shape[0] for x in q], never, 6), new_tokens(fresh, [c.shape[0] for c in conv], never, 6),
          "second turn")
    # the continued call starts with an empty history: a sequence spanning the two turns does not match
    first = new_tokens(got, [x.shape[0] for x in q], never, 6)[2][0]
    span = [rows[2][-1], first]
    past2 = model.generate(prompts, max_steps=N, temperature=0.0, decode=False, eos_token=eos_ids, stop_sequences=seqs,
                           return_past_key_values=True)[1]
    _, fin2 = model.generate(q, max_steps=2, temperature=0.0, decode=False, eos_token=[(first + 1) % 1000], stop_sequences=[span],
                             past_key_values=past2, return_finish=True)
    assert int(fin2.kept[2]) == 2          # not finished at step 0, where a match across the turns would have ended


def test_return_finish_decode_and_strings(dev):
    model = _diverse(dev)
    B, S = 5, 7
    emb = _emb(model, B, S, seed=146)
    plain = _plain(model, emb)
    eos_ids, seqs = _stops_from(plain, leave=4)
    ids, fin = _gen(model, emb, eos_ids, seqs)
    txt, fin_t = model.generate(emb, max_steps=N, temperature=0.0, eos_token=eos_ids, stop_sequences=seqs, return_finish=True)
    assert fin_t.reason == fin.reason and torch.equal(fin_t.kept, fin.kept) and set(fin.reason) == {"eos", "stop", "length"}
    for r in range(B):        # every string ends at the row's own kept count; the eos that finished a row is dropped
        n = int(fin.kept[r]) - (fin.reason[r] == "eos")
        assert txt[r] == model.tokenizer.decode([t for t in ids[r, :n].tolist() if t != model.image_token]), r
    # a string stop sequence is tokenised by the model's tokenizer: the call with its ids; ids outside the vocabulary are refused
    # before anything runs
    as_ids = [int(t) for t in model.tokenizer.encode("ab")]
    assert as_ids and all(0 <= t < 1056 for t in as_ids)
    out_s, fin_s = model.generate(emb, max_steps=N, temperature=0.0, decode=False, stop_sequences=["ab", seqs[0]], return_finish=True)
    out_i, fin_i = model.generate(emb, max_steps=N, temperature=0.0, decode=False, stop_sequences=[as_ids, seqs[0]], return_finish=True)
    assert torch.equal(out_s, out_i) and fin_s.reason == fin_i.reason and "stop" in fin_s.reason and fin_s.index == fin_i.index
    for kw in (dict(eos_token=[model.eos_token, 1056]), dict(stop_sequences=[[3, 2000]])):
        with pytest.raises(ValueError):
            model.generate(emb, max_steps=N, temperature=0.0, **kw)
    for kw in (dict(num_beams=2), dict(return_scores=True)):
        with pytest.raises(NotImplementedError):
            model.generate(emb, max_steps=N, stop_sequences=seqs, **kw)
