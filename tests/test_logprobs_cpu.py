"""Token log-probabilities, host side (DESIGN.md "Token log-probabilities"): the host statement
magma_amd.sampling.token_logprobs against torch.log_softmax + gather + a stable sort on crafted rows (exact ties at the n-th
logit and at the maximum), generate(return_logprobs=True, top_logprobs=3) on the tiny random GPT-J of the CPU generate tests
against the statement applied to the logits that LM returned, and the argument checks.  No GPU: the device kernel is tested
against the same statement in tests/test_logprobs_gpu.py."""
import pytest
import torch

from magma_amd.sampling import TokenLogprobs, check_logprob_args, generate, mask_logprobs, token_logprobs
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma

N_STEPS = 10


def _crafted():
    """Rows of 12 logits: distinct values, the maximum duplicated, three copies of the 3rd value, all equal, and a -inf entry."""
    g = torch.Generator().manual_seed(5)
    a = torch.randn(12, generator=g)
    b = a.clone()
    b[9] = b[2] = a.max() + 1.0                     # the maximum twice: ids 2, then 9
    c = torch.arange(12, dtype=torch.float32).flip(0).clone()
    c[[1, 6, 10]] = float(c[2])                         # values 11, then 9 four times (ids 1, 2, 6, 10), then 8, ...
    d = torch.full((12,), 0.25)
    e = a.clone()
    e[4] = float("-inf")
    return torch.stack([a, b, c, d, e])


@pytest.mark.parametrize("n_top", [0, 1, 3, 5, 12])
def test_host_statement_on_crafted_rows(n_top):
    x = _crafted()
    tok = torch.tensor([3, 9, 6, 11, 4])
    lp, ids, tl = token_logprobs(x, tok, n_top)
    ls = torch.log_softmax(x.double(), -1)
    assert lp.dtype == torch.float64 and torch.equal(lp, ls.gather(1, tok[:, None])[:, 0])
    assert lp[4] == float("-inf")                   # a token whose logit is -inf
    order = torch.sort(x.double(), dim=-1, descending=True, stable=True)[1][:, :n_top]
    assert ids.dtype == torch.int64 and torch.equal(ids, order) and torch.equal(tl, ls.gather(1, order))
    if n_top >= 1:
        assert torch.equal(ids[:, 0], x.argmax(-1)) and ids[1, 0] == 2 and ids[3, 0] == 0       # the first maximum
    if n_top >= 3:
        assert ids[2, :3].tolist() == [0, 1, 2]     # of the four ties at the 2nd to 5th place the lower ids come first
        assert ids[3, :n_top].tolist() == list(range(n_top))
    if n_top >= 5:
        assert ids[2, :5].tolist() == [0, 1, 2, 6, 10]
    # monotone in the log-probability
    assert bool((tl[:, :-1] >= tl[:, 1:]).all())


def test_host_statement_token_outside_and_bounds():
    x = _crafted()
    lp, ids, _ = token_logprobs(x, torch.tensor([-1, 12, 0, 11, 100]), 2)
    assert lp[:2].tolist() == [float("-inf")] * 2 and lp[4] == float("-inf") and torch.isfinite(lp[2:4]).all()
    assert ids.shape == (5, 2)
    for bad in (-1, 13, 21):
        with pytest.raises(ValueError):
            token_logprobs(x, torch.zeros(5, dtype=torch.int64), bad)


def test_masking_past_count():
    lp, ti, tl = torch.ones(2, 4), torch.ones(2, 4, 3, dtype=torch.int64), torch.ones(2, 4, 3)
    r = mask_logprobs(torch.zeros(2, 4, dtype=torch.int64), lp, ti, tl, torch.tensor([4, 1]))
    assert isinstance(r, TokenLogprobs) and r.count.tolist() == [4, 1]
    assert bool((r.logprobs[0] == 1).all()) and r.logprobs[1].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert bool((r.top_ids[1, 1:] == -1).all()) and bool((r.top_logprobs[1, 1:] == float("-inf")).all())
    assert bool((r.top_ids[1, 0] == 1).all()) and bool((lp == 1).all())         # the inputs are left alone


class _Recording(_HostMagma):
    """_HostMagma whose LM keeps the last-position logits of every call."""

    def __init__(self, lm):
        super().__init__(lm)
        self.seen = []
        inner = self.lm.forward

        def forward(**kw):
            o = inner(**kw)
            self.seen.append(o.logits[:, -1, :].float().clone())
            return o

        self.lm.forward = forward


@pytest.fixture(scope="module")
def tiny():
    model = _tiny_gptj(seed=4, eos_bias=1.5)
    emb = torch.randn(3, 5, 32, generator=torch.Generator().manual_seed(11))
    return model, emb


def _expect(seen, tokens, k):
    """The statement on the recorded logits, step by step, in the result's dtypes."""
    n = tokens.shape[1]
    vals = [token_logprobs(seen[i], tokens[:, i], k) for i in range(n)]
    return (torch.stack([v[0] for v in vals], 1).float(), torch.stack([v[1] for v in vals], 1),
            torch.stack([v[2] for v in vals], 1).float())


@pytest.mark.parametrize("mode", ["greedy", "sampled", "sampled_rules"])
def test_generate_equals_statement_on_the_lm_logits(tiny, mode):
    lm, emb = tiny
    kw = dict(temperature=0.0) if mode == "greedy" else dict(temperature=0.9, top_k=6)
    if mode == "sampled_rules":         # the processors change the selection, not the distribution the numbers are taken from
        kw.update(repetition_penalty=1.6, no_repeat_ngram_size=2)
    model = _Recording(lm)
    torch.manual_seed(21)
    out, lps = generate(model, emb, max_steps=N_STEPS, decode=False, eos_token=EOS, stop_on_eos=False, return_logprobs=True,
                        top_logprobs=3, **kw)
    torch.manual_seed(21)
    plain = generate(_HostMagma(lm), emb, max_steps=N_STEPS, decode=False, eos_token=EOS, stop_on_eos=False, **kw)
    assert torch.equal(out, plain)                  # the flags change no token
    S = emb.shape[1]
    assert torch.equal(lps.tokens, out[:, S:]) and lps.count.tolist() == [N_STEPS] * 3 and len(model.seen) == N_STEPS
    lp, ids, tl = _expect(model.seen, lps.tokens, 3)
    assert lps.logprobs.dtype == torch.float32 and lps.top_ids.dtype == torch.int64 and lps.top_logprobs.dtype == torch.float32
    assert torch.equal(lps.logprobs, lp) and torch.equal(lps.top_ids, ids) and torch.equal(lps.top_logprobs, tl)
    assert lps.top_ids.shape == (3, N_STEPS, 3) and bool((lps.logprobs <= 0).all())
    if mode == "greedy":                            # the greedy token is entry 0 of the alternatives
        assert torch.equal(lps.top_ids[:, :, 0], lps.tokens) and torch.equal(lps.top_logprobs[:, :, 0], lps.logprobs)
    # top_logprobs alone implies return_logprobs; return_logprobs alone gives empty lists
    torch.manual_seed(21)
    _, only = generate(_HostMagma(lm), emb, max_steps=N_STEPS, decode=False, eos_token=EOS, stop_on_eos=False, return_logprobs=True, **kw)
    assert torch.equal(only.logprobs, lps.logprobs) and only.top_ids.shape == (3, N_STEPS, 0)
    torch.manual_seed(21)
    assert len(generate(_HostMagma(lm), emb, max_steps=N_STEPS, decode=False, eos_token=EOS, stop_on_eos=False, top_logprobs=2, **kw)) == 2


def test_per_row_stopping_masks_past_count(tiny):
    lm, emb = tiny
    plain = generate(_HostMagma(lm), emb, max_steps=N_STEPS, temperature=0.0, decode=False, eos_token=EOS, stop_on_eos=False)[:, 5:]
    rows = plain.tolist()
    eos_ids = [rows[0][2], rows[1][5]]              # row 0 finishes by step 2, row 1 by step 5
    model = _Recording(lm)
    out, fin, lps = generate(model, emb, max_steps=N_STEPS, temperature=0.0, decode=False, eos_token=eos_ids, return_finish=True,
                             return_logprobs=True, top_logprobs=3)
    n = out.shape[1] - 5
    assert torch.equal(lps.count, fin.kept) and len(set(fin.kept.tolist())) > 1 and int(fin.kept.min()) < n
    assert torch.equal(lps.tokens, out[:, 5:])
    lp, ids, tl = _expect(model.seen, lps.tokens, 3)
    for r in range(3):
        k = int(fin.kept[r])
        assert torch.equal(lps.logprobs[r, :k], lp[r, :k]) and torch.equal(lps.top_ids[r, :k], ids[r, :k])
        assert torch.equal(lps.top_logprobs[r, :k], tl[r, :k])
        assert bool((lps.logprobs[r, k:] == 0.0).all()) and bool((lps.top_ids[r, k:] == -1).all())
        assert bool((lps.top_logprobs[r, k:] == float("-inf")).all())


def test_argument_validation(tiny):
    lm, emb = tiny
    assert check_logprob_args() is None and check_logprob_args(True) == 0 and check_logprob_args(False, 4) == 4
    assert check_logprob_args(True, 20, vocab=20) == 20
    for bad in (dict(top_logprobs=-1), dict(top_logprobs=21), dict(top_logprobs=True), dict(top_logprobs=2.0),
                dict(top_logprobs=8, vocab=7), dict(return_logprobs=1)):
        with pytest.raises(ValueError):
            check_logprob_args(**bad)

    class _Never(_HostMagma):           # every refusal comes before the LM is called
        def __init__(self, lm):
            super().__init__(lm)
            self.lm.forward = lambda **kw: pytest.fail("the LM ran")

    model = _Never(lm)
    for bad in (dict(top_logprobs=21), dict(top_logprobs=-2), dict(top_logprobs=V + 1), dict(top_logprobs="3")):
        with pytest.raises(ValueError):
            generate(model, emb, max_steps=3, temperature=0.0, **bad)
    for beam in (dict(num_beams=2), dict(return_scores=True)):
        for flags in (dict(return_logprobs=True), dict(top_logprobs=2)):
            with pytest.raises(NotImplementedError):
                generate(model, emb, max_steps=3, **beam, **flags)
