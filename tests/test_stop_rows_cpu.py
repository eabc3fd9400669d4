"""Per-row stopping: the host statement (magma_amd.sampling.stop_update, inside the generic host loop of generate()) against the
installed transformers' generate() -- eos_token_id as a list, pad_token_id = the first of them, and a StoppingCriteria that
matches id sequences against the generated ids -- on the tiny random GPT-J of tests/test_beam_search_cpu.py driven by
inputs_embeds; min_new_tokens with two eos ids against MinNewTokensLengthLogitsProcessor; the argument checks.  No GPU: the
device kernel is tested against the same host statement in tests/test_stop_rows_gpu.py."""
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import (REASON_EOS, REASON_NONE, REASON_STOP, check_stop_args, finish_from_record, generate, process_logits,
                                stop_update)
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma, _same_bits

N_STEPS, B = 14, 5


def _criteria(seqs, eos_ids, log):
    """transformers' StoppingCriteria over id sequences: a row is done when its generated ids end with one of ``seqs``.  ``log``
    receives, per row, the first (step, reason, index) at which transformers' own eos test or this one fired."""
    from transformers import StoppingCriteria

    class _Seqs(StoppingCriteria):
        def __call__(self, input_ids, scores, **kw):
            n = input_ids.shape[1]
            hit = [next((j for j, q in enumerate(seqs) if len(q) <= n and row[n - len(q):].tolist() == list(q)), None) for row in input_ids]
            for r, j in enumerate(hit):
                last = int(input_ids[r, -1])
                if r not in log and (last in eos_ids or j is not None):
                    log[r] = (n - 1, "eos", eos_ids.index(last)) if last in eos_ids else (n - 1, "stop", j)
            return torch.tensor([j is not None for j in hit], dtype=torch.bool, device=input_ids.device)

    return _Seqs()


def _hf(model, emb, eos_ids, seqs, rules):
    from transformers import StoppingCriteriaList
    log = {}
    out = model.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), do_sample=False,
                         max_new_tokens=N_STEPS, eos_token_id=list(eos_ids), pad_token_id=eos_ids[0],
                         stopping_criteria=StoppingCriteriaList([_criteria(seqs, list(eos_ids), log)]), **rules)
    return out, log


def _ours(model, emb, eos_ids, seqs, rules, **kw):
    out, fin = generate(_HostMagma(model), emb, max_steps=N_STEPS, temperature=0.0, eos_token=list(eos_ids), stop_sequences=seqs,
                        decode=False, return_finish=True, **rules, **kw)
    return out[:, emb.shape[1]:], fin


def _plain(model, emb, rules):
    return generate(_HostMagma(model), emb, max_steps=N_STEPS, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False,
                    **rules)[:, emb.shape[1]:]


def _outcome(rows, eos_ids, seqs):
    """Per row of the plain run: (step, reason) at which these items would first finish it, or None."""
    out = []
    for row in rows:
        hit = None
        for t in range(len(row)):
            if row[t] in eos_ids:
                hit = (t, "eos")
            elif any(len(q) <= t + 1 and row[t + 1 - len(q): t + 1] == q for q in seqs):
                hit = (t, "stop")
            if hit:
                break
        out.append(hit)
    return out


def _stops_from(plain, leave=None):
    """Stop items that bite on the plain run's rows at spread-out steps: every row in turn (row ``leave`` excepted: nothing may
    finish it) contributes one item taken from its own tokens -- an eos id, or a stop sequence of two or three tokens -- namely
    the one after which the rows finish for both reasons, then an eos id from an even row and a sequence from an odd one, then
    at the most distinct steps, in the largest number and at the earliest step.  At most 8 eos ids and 16 sequences."""
    rows = [r.tolist() if torch.is_tensor(r) else list(r) for r in plain]

    def score(got, preferred):
        return len({g[1] for g in got if g}), preferred, len({g[0] for g in got if g}), sum(g is not None for g in got)

    eos_ids, seqs = [], []
    for r, row in enumerate(rows):
        if r == leave:
            continue
        best = (score(_outcome(rows, eos_ids, seqs), 0) + (0,), eos_ids, seqs)
        for t in range(len(row)):
            for cand in [[row[t]]] + [row[t + 1 - n: t + 1] for n in (2, 3) if n <= t + 1]:
                is_eos = len(cand) == 1
                e, q = (eos_ids + cand, seqs) if is_eos else (eos_ids, seqs + [cand])
                if len(e) > 8 or len(q) > 16 or cand[0] in eos_ids or cand in seqs:
                    continue
                got = _outcome(rows, e, q)
                if leave is not None and got[leave] is not None:
                    continue
                sc = score(got, int(is_eos == (r % 2 == 0))) + (-t,)
                if sc > best[0]:
                    best = (sc, e, q)
        eos_ids, seqs = best[1], best[2]
    assert eos_ids, rows
    return eos_ids, seqs


# model seed, input seed, rules, the row nothing aims at: chosen so that transformers' own run meets the preconditions below
CASES = {"greedy": (4, 11, {}, None), "penalty": (6, 11, dict(repetition_penalty=1.7), None),
         "penalty_length": (6, 11, dict(repetition_penalty=1.7), 3)}


@pytest.mark.parametrize("case", list(CASES))
def test_generic_loop_equals_transformers_generate(case):
    pytest.importorskip("transformers")
    m_seed, e_seed, rules, leave = CASES[case]
    model = _tiny_gptj(seed=m_seed, eos_bias=1.5)
    emb = torch.randn(B, 5, 32, generator=torch.Generator().manual_seed(e_seed))
    eos_ids, seqs = _stops_from(_plain(model, emb, rules), leave)
    ref, log = _hf(model, emb, eos_ids, seqs, rules)
    # preconditions, on transformers' run alone
    steps = {v[0] for v in log.values()}
    assert len(steps) >= 3, (log, "rows must finish at three distinct steps or more")
    assert {v[1] for v in log.values()} == {"eos", "stop"}, log
    assert (len(log) < B) == (leave is not None), (log, "a row that never finishes, in the length case only")
    got, fin = _ours(model, emb, eos_ids, seqs, rules)
    assert got.shape == ref.shape and torch.equal(got, ref), (eos_ids, seqs, got, ref)
    width = N_STEPS if len(log) < B else max(steps) + 1
    assert got.shape[1] == width and (leave is not None or width < N_STEPS)
    for r in range(B):
        step, why, idx = log.get(r, (width - 1, "length", -1))
        assert (int(fin.kept[r]), fin.reason[r], fin.index[r]) == (step + 1, why, idx), (r, fin, log)
        assert bool((got[r, step + 1:] == eos_ids[0]).all())
    # stop_on_eos=False: the same rows, padded to the full width
    full, fin_full = _ours(model, emb, eos_ids, seqs, rules, stop_on_eos=False)
    assert full.shape[1] == N_STEPS and torch.equal(full[:, :width], got) and bool((full[:, width:][fin.kept < width] == eos_ids[0]).all())
    assert fin_full.reason == fin.reason and fin_full.index == fin.index


def test_stop_per_row_with_one_eos_id_is_transformers_plain_rule():
    """stop_per_row=True and nothing else: transformers' generate() with one eos id (rows padded, the batch ends when all are done)."""
    pytest.importorskip("transformers")
    model = _tiny_gptj(seed=4, eos_bias=1.5)
    emb = torch.randn(B, 5, 32, generator=torch.Generator().manual_seed(11))
    ref = model.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), do_sample=False,
                         max_new_tokens=N_STEPS, eos_token_id=EOS, pad_token_id=EOS)
    got = generate(_HostMagma(model), emb, max_steps=N_STEPS, temperature=0.0, eos_token=EOS, decode=False, stop_per_row=True)[:, 5:]
    assert 1 < ref.shape[1] < N_STEPS and torch.equal(got, ref)
    old = generate(_HostMagma(model), emb, max_steps=N_STEPS, temperature=0.0, eos_token=EOS, decode=False)[:, 5:]
    assert old.shape[1] > got.shape[1]          # the reference's rule waits for a step at which EVERY row selects eos


def test_stop_update_rule_by_rule():
    hist = torch.tensor([[5, 6, 7, 0], [5, 6, 9, 0], [1, 5, 6, 0], [6, 7, 8, 0]])
    none = [REASON_NONE, -1]
    done, why = stop_update(hist, 2, torch.zeros(4, dtype=torch.bool), [3, 7], [[6, 9], [9], [5, 6], [1, 5, 6], [9, 9, 9, 9]])
    assert done.tolist() == [True, True, True, False]
    assert why.tolist() == [[REASON_EOS, 1], [REASON_STOP, 0], [REASON_STOP, 2], none]      # lowest index; a suffix of another
    # eos is tested first; a done row is not looked at again; a sequence longer than step + 1 cannot match
    done, why = stop_update(hist, 1, torch.tensor([False, True, False, False]), [6], [[5, 6], [0, 1, 5]])
    assert done.tolist() == [True, True, False, False] and why.tolist() == [[REASON_EOS, 0], none, none, none]
    assert stop_update(hist, 0, torch.zeros(4, dtype=torch.bool), [3], [[5, 6], [0, 5]])[0].tolist() == [False] * 4
    fin = finish_from_record([[2, REASON_EOS * 256 + 1], [-1, 0], [0, REASON_STOP * 256 + 15]], 4)
    assert fin.kept.tolist() == [3, 4, 1] and fin.reason == ["eos", "length", "stop"] and fin.index == [1, -1, 15]


def test_min_new_tokens_bans_every_eos_id():
    pytest.importorskip("transformers")
    from transformers import MinNewTokensLengthLogitsProcessor
    g = torch.Generator().manual_seed(5)
    a, b = 7, 30
    for n in (1, 4):
        for step in (0, n - 1, n, n + 3):
            x = torch.randn(4, V, generator=g)
            hist = torch.randint(0, V, (4, step), generator=g)
            ref = MinNewTokensLengthLogitsProcessor(0, n, [a, b])(hist, x.clone())
            got = process_logits(x, torch.cat([hist, torch.zeros(4, 2, dtype=torch.int64)], 1), step, min_new_tokens=n, eos_token=[a, b])
            assert _same_bits(got, ref)
            assert bool((got[:, [a, b]] == float("-inf")).all()) == (step < n)


def test_argument_validation():
    assert check_stop_args(EOS) is None and check_stop_args(EOS, None, False) is None
    assert check_stop_args(EOS, None, True) == dict(eos_ids=(EOS,), stop_seqs=())
    assert check_stop_args([EOS]) == dict(eos_ids=(EOS,), stop_seqs=())
    ok = check_stop_args(list(range(8)), [[1] * 16] * 16, None, V)
    assert len(ok["eos_ids"]) == 8 and len(ok["stop_seqs"]) == 16 and len(ok["stop_seqs"][0]) == 16
    assert check_stop_args(EOS, ["ab", [3]], encode=lambda s: [ord(c) % V for c in s])["stop_seqs"] == ((ord("a") % V, ord("b") % V), (3,))
    bad = [dict(eos_token=list(range(9))), dict(eos_token=[]), dict(stop_sequences=[[1]] * 17), dict(stop_sequences=[[]]),
           dict(stop_sequences=[[1] * 17]), dict(eos_token=[EOS, V]), dict(eos_token=[-1]), dict(stop_sequences=[[V]]),
           dict(stop_sequences=[[1, -2]]), dict(stop_sequences=[[1.5]]), dict(stop_sequences="text"), dict(stop_sequences=["text"]),
           dict(eos_token=[EOS, 3], stop_per_row=False), dict(stop_sequences=[[1]], stop_per_row=False), dict(stop_per_row="yes")]
    for kw in bad:
        with pytest.raises(ValueError):
            check_stop_args(**{"eos_token": EOS, "vocab": V, **kw})

    class _NoModel:            # the checks run before generate() touches the model
        eos_token = EOS
        training = False
        lm = SimpleNamespace(config=SimpleNamespace(vocab_size=V))

    emb = torch.zeros(1, 2, 8)
    for kw in bad:
        with pytest.raises(ValueError):
            generate(_NoModel(), emb, max_steps=2, **kw)
    for kw in [dict(eos_token=[EOS, 3]), dict(stop_sequences=[[1, 2]]), dict(stop_per_row=True), dict(return_finish=True)]:
        for beam in (dict(num_beams=2), dict(return_scores=True)):
            with pytest.raises(NotImplementedError):
                generate(_NoModel(), emb, max_steps=2, **kw, **beam)
    with pytest.raises(TypeError):          # keyword-only
        generate(_NoModel(), emb, 2, 0.0, 0, 0.9, EOS, False, True, None, None, None, 1, 1.0, False, 1, False, None, False, [[1]])
