"""The rules, constraint and log-probability launches of a slot session (DESIGN.md "Choosing over a request stream"):
ops.logits_process_slots, ops.logits_process_constrained_slots and ops.token_logprobs_slots against their flat twins.

The statement under test: an occupied row r of a slot launch gives the BITS its flat twin gives when it is launched alone on row
r with the occupant's window unrolled to column 0 (sampling.slot_tokens) and state[0] = n; an idle row is not touched.  One case
per kernel is also compared with the host statements the flat kernels are tested against (process_logits and constrain_logits
bit for bit, token_logprobs under test_logprobs_gpu's bound).

Every ring is hostile outside the windows: behind a window stands the token that continues the row's walk through its trie, in
front of it the trie's tokens [5, 6, 9], and the rest alternates (the window's last token, a token the window lacks) -- an n-gram
completion and a penalty target.  ``test_the_ring_is_hostile`` shows that a launch which read the whole ring would differ."""
import pytest
import torch

from device_indices import Guarded, Operands, same_bits
from test_constrained_gpu import _tries
from test_logprobs_gpu import _within

pytestmark = pytest.mark.gpu

HC = 32                     # ring columns
LPC = 24                    # log-probability columns: fewer than the ring has, so n = 31 lies beyond them
EOS = (3, 4)
SENT = -77.0
# (state[0], n per row by r % len): column (s - 1) % HC is the newest token's.  s = 5 / 37: column 4, so n > 5 wraps; s = 1: column
# 0, every n > 1 wraps; s = 32: column 31, nothing wraps; n = HC fills the ring.
STATES = [(5, (1, 31, 7, 3, 6, HC, 2, 12)), (37, (31, 1, 9, 5, 20)), (1, (2, 1, 31, 17, 4)), (32, (31, 1, 32, 8, 3))]
RULES = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
SUPPRESS = (2, 6)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _track(V, r, n):
    """n tokens for row r: deep along the 64-token sequence, a leaf then eos, the terminal inner node [5, 6], off the trie."""
    a, b, s64 = _tries(V)
    pad = [EOS[0]] * HC
    rows = [s64, [5, 6, 9] + pad, [5, 6] + pad, [5, 4, 5, 6, 9, 5, 6] + pad, s64]
    return rows[r % len(rows)][:n]


def _case(R, V, s, ns, seed=0, idle=()):
    """One launch's host operands: logits [R, V + 7] (sentinel padding; NaN rows where idle), ring [R, HC], slot, finish, tries,
    begin and n per row."""
    a, b, s64 = _tries(V)
    g = torch.Generator().manual_seed(seed * 1000 + R * 7 + V + s)
    full = torch.full((R, V + 7), 123.25)
    full[:, :V] = torch.randn(R, V, generator=g) * 3
    full[:, 0], full[:, V - 1], full[:, 5] = 0.5, float("-inf"), -0.0
    col = (s - 1) % HC
    ring = torch.zeros(R, HC, dtype=torch.int64)
    slot, finish, n_of, begins = torch.zeros(R, 2, dtype=torch.int32), torch.zeros(R, 2, dtype=torch.int32), [], []
    for r in range(R):
        n = ns[r % len(ns)]
        begin = (col - (n - 1)) % HC
        toks = _track(V, r, n)
        spare = next(t for t in range(10, V) if t not in toks and t not in EOS)
        hostile = [s64[n] if s64[n] != V - 1 else spare] + [toks[-1], spare] * HC       # (column V - 1 is -inf: no penalty shows)
        out = hostile[: HC - n]
        if len(out) >= 4:
            out[-3:] = [5, 6, 9]            # in front of the window (ring order): the start of another walk
        for i, t in enumerate(toks + out):
            ring[r, (begin + i) % HC] = t
        slot[r] = torch.tensor([begin, 99])
        finish[r] = torch.tensor([-1, 0])
        n_of.append(n)
        begins.append(begin)
    for r in idle:
        finish[r] = torch.tensor([max(s - 2, 0), 0x100])
        full[r] = float("nan")
    tries = [b if r % 4 == 3 else a for r in range(R)]
    return dict(full=full, ring=ring, slot=slot, finish=finish, tries=tries, n=n_of, begin=begins, s=s, V=V, R=R, idle=set(idle))


def _state(dev, s):
    return torch.tensor([s, -1], dtype=torch.int32, device=dev)


def _rule_kw(dev, rules, constrained):
    kw = dict(eos=EOS[0], eos_more=torch.tensor(EOS[1:], dtype=torch.int32, device=dev))
    if rules:
        kw.update(repetition_penalty=RULES["repetition_penalty"], min_new_tokens=RULES["min_new_tokens"],
                  suppress=torch.tensor(SUPPRESS, dtype=torch.int32, device=dev))
        if not constrained:
            kw["no_repeat_ngram_size"] = RULES["no_repeat_ngram_size"]
    return kw


def _trie_bufs(dev, tries, R):
    from magma_amd import ops
    from magma_amd.sampling import trie_forest
    table, roots = trie_forest(tries)
    return table.to(dev), roots.to(dev), ops.trie_path(R, dev)


def _unrolled(c, r):
    from magma_amd.sampling import slot_tokens
    flat = torch.full((1, HC), -5, dtype=torch.int64)       # (behind the n tokens: ids no rule accepts)
    toks = slot_tokens(c["ring"][r], c["begin"][r], c["s"], HC)
    assert toks.numel() == c["n"][r]
    flat[0, : toks.numel()] = toks
    return flat


def _process(dev, c, rules, constrained, path=None, whole_ring=False):
    """(slot launch's logits, the flat twin's row by row) as host tensors."""
    from magma_amd import ops
    V, R = c["V"], c["R"]
    kw = _rule_kw(dev, rules, constrained)
    x = c["full"].to(dev)
    ring, slot, finish = c["ring"].to(dev), c["slot"].to(dev), c["finish"].to(dev)
    if constrained:
        table, roots, fresh = _trie_bufs(dev, c["tries"], R)
        ops.logits_process_constrained_slots(x[:, :V], _state(dev, c["s"]), ring, table, roots, fresh if path is None else path,
                                             slot, finish, **kw)
    else:
        ops.logits_process_slots(x[:, :V], _state(dev, c["s"]), ring, slot, finish, **kw)
    want = c["full"].clone()
    for r in range(R):
        if r in c["idle"]:
            continue
        y = c["full"][r:r + 1].to(dev)
        hist = (c["ring"][r:r + 1] if whole_ring else _unrolled(c, r)).to(dev)
        st = _state(dev, HC if whole_ring else c["n"][r])
        if constrained:
            t1, r1, p1 = _trie_bufs(dev, [c["tries"][r]], 1)
            ops.logits_process_constrained(y[:, :V], st, hist, t1, r1, p1, **kw)
        else:
            ops.logits_process(y[:, :V], st, hist, **kw)
        want[r] = y[0].cpu()
    return x.cpu(), want


def _idle_rows(R):
    return () if R == 1 else tuple(range(1, R, 3))


@pytest.mark.parametrize("V", [97, 50258])
@pytest.mark.parametrize("R", [1, 5, 16])
@pytest.mark.parametrize("constrained", [False, True])
def test_slot_rules_equal_the_flat_twin_on_the_unrolled_window(dev, constrained, R, V):
    changed = 0
    for k, (s, ns) in enumerate(STATES):
        c = _case(R, V, s, ns[k % 2:] + ns[: k % 2], seed=k, idle=_idle_rows(R))
        for rules in (True, False) if constrained else (True,):
            got, want = _process(dev, c, rules, constrained)
            assert torch.equal(_bits(got), _bits(want)), (s, rules, (_bits(got) != _bits(want)).any(1).nonzero().flatten().tolist())
            changed += int(not torch.equal(_bits(want), _bits(c["full"])))
    assert changed >= len(STATES)


def _host_rules(c, r, hist, n, constrained):
    from magma_amd.sampling import constrain_logits, process_logits
    V = c["V"]
    x = process_logits(c["full"][r:r + 1, :V], hist, n, eos_token=list(EOS), repetition_penalty=RULES["repetition_penalty"],
                       min_new_tokens=RULES["min_new_tokens"], suppress_tokens=SUPPRESS,
                       no_repeat_ngram_size=0 if constrained else RULES["no_repeat_ngram_size"])
    return constrain_logits(x, hist, n, [c["tries"][r]], EOS) if constrained else x


@pytest.mark.parametrize("constrained", [False, True])
def test_the_ring_is_hostile(constrained):
    """On the host statements alone: the rules over the WHOLE ring from column 0, over the window plus the column behind it, and
    over the window from one column early each differ from the rules over the window -- in three of four cases for the plain
    rules, in half of them under the constraint (a row that has left its trie keeps the eos ids whatever else it reads): the tests
    above cannot pass by reading beyond a window."""
    from magma_amd.sampling import slot_tokens
    differ = rows = 0
    for k, (s, ns) in enumerate(STATES):
        c = _case(8, 97, s, ns, seed=k)
        for r in range(8):
            n, begin = c["n"][r], c["begin"][r]
            if n >= HC - 1:
                continue
            want = _host_rules(c, r, slot_tokens(c["ring"][r], begin, s, HC)[None], n, constrained)
            ring = c["ring"][r]
            longer = ring[(begin + torch.arange(n + 1)) % HC][None]
            early = ring[(begin - 1 + torch.arange(n + 1)) % HC][None]
            wrong = [_host_rules(c, r, ring[None], HC, constrained), _host_rules(c, r, longer, n + 1, constrained),
                     _host_rules(c, r, early, n + 1, constrained)]
            differ += sum(not torch.equal(_bits(want), _bits(w)) for w in wrong)
            rows += 3
    print(f"hostile ring: {differ} of {rows} wrong windows change the result")
    assert differ >= rows * (0.5 if constrained else 0.75), (differ, rows)


def test_slot_rules_equal_the_host_statements(dev):
    from magma_amd.sampling import slot_tokens
    V, R = 1056, 5
    s, ns = STATES[0]
    c = _case(R, V, s, ns, seed=9, idle=(2,))
    for constrained in (False, True):
        got, _ = _process(dev, c, True, constrained)
        for r in range(R):
            if r in c["idle"]:
                assert torch.equal(_bits(got[r]), _bits(c["full"][r]))
                continue
            x = _host_rules(c, r, slot_tokens(c["ring"][r], c["begin"][r], s, HC)[None], c["n"][r], constrained)
            assert torch.equal(_bits(got[r, :V]), _bits(x[0])), (constrained, r)
            assert torch.equal(_bits(got[r, V:]), _bits(c["full"][r, V:]))


def test_path_cache_of_other_occupants_and_tables_is_invisible(dev):
    """One path buffer through launches whose windows, occupants and tables change: the results of fresh buffers every time; then
    arbitrary numbers in it."""
    V, R = 97, 5
    from magma_amd import ops
    path = ops.trie_path(R, dev)
    for k, (s, ns) in enumerate(STATES + STATES[:2]):
        c = _case(R, V, s, ns[k % 3:] + ns[: k % 3], seed=k)
        if k % 2:           # other tries: other node numbers and roots in the table
            c["tries"] = c["tries"][::-1]
        got, want = _process(dev, c, False, True, path=path)
        assert torch.equal(_bits(got), _bits(want)), k
    g = torch.Generator().manual_seed(0)
    path.copy_(torch.randint(-5, 4000, path.shape, generator=g).to(torch.int32))
    got, want = _process(dev, c, False, True, path=path)
    assert torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------- log-probabilities
@pytest.mark.parametrize("V", [97, 50258])
@pytest.mark.parametrize("R", [1, 5, 16])
@pytest.mark.parametrize("n_top", [0, 3])
def test_slot_logprobs_equal_the_flat_twin(dev, n_top, R, V):
    from magma_amd import ops
    from magma_amd.sampling import token_logprobs
    written = 0
    for k, (s, ns) in enumerate(STATES):
        c = _case(R, V, s, ns, seed=k, idle=_idle_rows(R))
        x = c["full"].to(dev)
        tok = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(k)).to(dev)
        lp = torch.full((R, LPC), SENT, device=dev)
        tid = torch.full((R, LPC, n_top), int(SENT), dtype=torch.int32, device=dev)
        tlp = torch.full((R, LPC, n_top), SENT, device=dev)
        ops.token_logprobs_slots(x[:, :V], tok, lp, tid if n_top else None, tlp if n_top else None, _state(dev, s),
                                 c["slot"].to(dev), c["finish"].to(dev), HC)
        w_lp, w_id, w_tl = torch.full_like(lp, SENT), torch.full_like(tid, int(SENT)), torch.full_like(tlp, SENT)
        for r in range(R):
            if r in c["idle"]:
                continue
            ops.token_logprobs(x[r:r + 1, :V], tok[r:r + 1], w_lp[r:r + 1], w_id[r:r + 1] if n_top else None,
                               w_tl[r:r + 1] if n_top else None, state=_state(dev, c["n"][r]))
            written += int(c["n"][r] < LPC)
        assert torch.equal(_bits(lp), _bits(w_lp)) and torch.equal(tid, w_id) and torch.equal(_bits(tlp), _bits(w_tl)), s
        assert torch.equal(_bits(x.cpu()), _bits(c["full"]))         # (NaN rows included: the logits are only read)
        if k == 0 and V == 97:      # the statement itself, at the columns that were written
            rows = [r for r in range(R) if r not in c["idle"] and c["n"][r] < LPC]
            r_lp, r_id, r_tl = token_logprobs(c["full"][rows, :V], tok.cpu()[rows], n_top)
            cols = torch.tensor([c["n"][r] for r in rows])
            _within(lp.cpu()[rows, cols], r_lp, V, f"slot lp R={R}")
            if n_top:
                assert torch.equal(tid.cpu()[rows, cols].long(), r_id)
                _within(tlp.cpu()[rows, cols], r_tl, V, f"slot top_lp R={R}")
    assert written >= 2


# ------------------------------------------------------------------------------------------- indices from device memory
def _guarded_launch(dev, c, which, table=None):
    """One launch of entry point ``which`` with every operand guard-banded; returns (Operands, the row -> expected map is the
    caller's)."""
    from magma_amd import ops
    V, R = c["V"], c["R"]
    tb, roots, path = _trie_bufs(dev, c["tries"], R)
    g = dict(x=Guarded.of(c["full"].to(dev)), ring=Guarded.of(c["ring"].to(dev)), slot=Guarded.of(c["slot"].to(dev)),
             finish=Guarded.of(c["finish"].to(dev)), table=Guarded.of(tb if table is None else table.to(dev)),
             roots=Guarded.of(roots), path=Guarded.of(path), lp=Guarded((R, LPC), torch.float32, dev),
             tid=Guarded((R, LPC, 3), torch.int32, dev), tlp=Guarded((R, LPC, 3), torch.float32, dev),
             tok=Guarded.of(torch.full((R,), 7, dtype=torch.int64, device=dev)), state=Guarded.of(_state(dev, c["s"])))
    o = Operands(**g).snapshot()
    kw = _rule_kw(dev, True, which == "constrained")
    x = g["x"].t[:, :V]
    if which == "process":
        ops.logits_process_slots(x, g["state"].t, g["ring"].t, g["slot"].t, g["finish"].t, **kw)
    elif which == "constrained":
        ops.logits_process_constrained_slots(x, g["state"].t, g["ring"].t, g["table"].t, g["roots"].t, g["path"].t, g["slot"].t,
                                             g["finish"].t, **kw)
    else:
        ops.token_logprobs_slots(x, g["tok"].t, g["lp"].t, g["tid"].t, g["tlp"].t, g["state"].t, g["slot"].t, g["finish"].t, HC)
    return o


@pytest.mark.parametrize("which", ["process", "constrained", "logprobs"])
@pytest.mark.parametrize("plant", ["begin=-1", "begin=cols", "finish past the ring", "corrupt trie header"])
def test_device_read_indices_never_leave_the_operands(dev, which, plant):
    """Row 1 carries the planted value.  A bad begin and a finish step >= 0 (whatever its size) make the row idle: none of its
    outputs is written.  A corrupt header takes every row off the trie.  The other rows equal the launch without the plant, and no
    guard band and no other operand changes."""
    from magma_amd.sampling import process_logits
    V, R = 97, 3
    s, ns = STATES[0]
    c = _case(R, V, s, ns, seed=4)
    clean = _guarded_launch(dev, c, which)
    torch.cuda.synchronize()
    clean_out = {n: clean[n].t.clone() for n in ("x", "lp", "tid", "tlp", "path")}
    table = None
    if plant == "begin=-1":
        c["slot"][1, 0] = -1
    elif plant == "begin=cols":
        c["slot"][1, 0] = HC
    elif plant == "finish past the ring":
        c["finish"][1, 0] = HC + 10 ** 6
    else:
        table, _, _ = _trie_bufs(dev, c["tries"], R)
        table = table.clone()
        table[:2] = torch.tensor([10 ** 6, 10 ** 6], dtype=torch.int32)
    o = _guarded_launch(dev, c, which, table=table)
    written = {}
    for name in ("x", "lp", "tid", "tlp", "path"):
        w = o.expected(name)
        rows = [r for r in range(R) if table is not None or r != 1]
        w[rows] = clean_out[name][rows]
        written[name] = w
    if table is not None and which == "constrained":
        # no trie: no walk (the path keeps what it held), and the rules' row keeps the eos ids alone -- the flat twin's statement
        del written["path"]
        for r in range(R):
            x = process_logits(c["full"][r:r + 1, :V], _unrolled(c, r)[:, : c["n"][r]], c["n"][r], eos_token=list(EOS),
                               repetition_penalty=RULES["repetition_penalty"], min_new_tokens=RULES["min_new_tokens"],
                               suppress_tokens=SUPPRESS)
            keep = torch.zeros(V, dtype=torch.bool)
            keep[list(EOS)] = True
            written["x"][r, :V] = x[0].masked_fill(~keep, float("-inf")).to(dev)
    o.check(f"{which}, {plant}", **written)


def test_refusals_return_before_any_launch(dev):
    """Every refusal of the three entry points: an error, and the operands keep their bits."""
    from magma_amd import lib, ops
    V, R = 97, 3
    s, ns = STATES[0]
    c = _case(R, V, s, ns, seed=5)
    x = c["full"].to(dev)
    ring, slot, finish, st = c["ring"].to(dev), c["slot"].to(dev), c["finish"].to(dev), _state(dev, s)
    table, roots, path = _trie_bufs(dev, c["tries"], R)
    tok = torch.zeros(R, dtype=torch.int64, device=dev)
    lp = torch.full((R, LPC), SENT, device=dev)
    L, stream = lib.load(), torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def process(**o):
        a = dict(ld=V + 7, R=R, V=V, state=p(st), hist=p(ring), ld_h=HC, hc=HC, pen=1.3, ngram=2, mn=0, ns=0, slot=p(slot), fin=p(finish))
        a.update(o)
        return L.mg_logits_process_slots_f32(p(x), a["ld"], a["R"], a["V"], a["state"], a["hist"], a["ld_h"], a["hc"], a["pen"],
                                             a["ngram"], a["mn"], EOS[0], None, a["ns"], 0, None, 0, a["slot"], a["fin"], stream)

    def constrained(**o):
        a = dict(ld=V + 7, V=V, hist=p(ring), hc=HC, pen=1.3, table=p(table), ints=table.numel(), roots=p(roots), path=p(path),
                 slot=p(slot), fin=p(finish))
        a.update(o)
        return L.mg_logits_process_constrained_slots_f32(p(x), a["ld"], R, a["V"], p(st), a["hist"], HC, a["hc"], a["pen"], 0, 0, EOS[0],
                                                         None, 0, None, 0, a["table"], a["ints"], a["roots"], a["path"], a["slot"],
                                                         a["fin"], stream)

    def logprobs(**o):
        a = dict(ld=V + 7, state=p(st), ld_lp=LPC, cols=LPC, n_top=0, slot=p(slot), fin=p(finish), hc=HC)
        a.update(o)
        return L.mg_token_logprobs_slots_f32(p(x), a["ld"], R, V, p(tok), a["state"], p(lp), a["ld_lp"], a["cols"], a["n_top"], None,
                                             None, a["slot"], a["fin"], a["hc"], stream)

    bad = [process(slot=None), process(fin=None), process(state=None), process(hist=None), process(hc=0), process(ld_h=HC - 1),
           process(ld=V - 1), process(R=0), process(pen=0.0), process(ngram=17), process(mn=-1), process(ns=1),
           constrained(slot=None), constrained(fin=None), constrained(table=None), constrained(ints=1), constrained(roots=None),
           constrained(path=None), constrained(hist=None), constrained(hc=0), constrained(pen=-1.0), constrained(ld=V - 1),
           logprobs(slot=None), logprobs(fin=None), logprobs(state=None), logprobs(hc=0), logprobs(cols=0), logprobs(ld_lp=LPC - 1),
           logprobs(n_top=21), logprobs(n_top=3), logprobs(ld=V - 1)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    assert b"mg_token_logprobs_slots_f32" in L.mg_last_error()
    assert same_bits(x.cpu(), c["full"]) and bool((lp == SENT).all()) and same_bits(path.cpu(), ops.trie_path(R, "cpu"))
    assert process() == 0 and constrained() == 0 and logprobs() == 0        # the same calls with nothing wrong are accepted
    torch.cuda.synchronize()
