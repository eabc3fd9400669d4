"""Helpers of the device-index contract tests (include/magma_hip.h "Device-resident indices"; DESIGN.md has the table): guarded
buffers, the planted index values and the snapshot compare.  A plain module like kernel_compare.py: no fixtures, no settings.

Every operand a kernel reaches through a device-resident index sits in a ``Guarded`` buffer: GUARD elements of a NaN bit pattern in
front of it and behind it, and the same pattern inside it wherever a correct kernel must not read (and in every output before the
launch).  The pattern is the 16-bit word 0x7FC1 repeated: a quiet NaN with a payload as bf16, a NaN as fp32 (0x7FC17FC1), and as
int32 / int64 a positive value far outside every index range of these tests.

The planted values lie at most two units outside their range (OUTSIDE), so that even a kernel without any guard stays inside the
test's own allocation: the farthest stray access is two cache positions of 256 elements (512 elements), two history columns or two
logits ids from the operand -- the 4096-element guard holds all of them."""
import torch

BF16 = torch.bfloat16
NAN16 = 0x7FC1                  # a quiet bf16 NaN with a payload
GUARD = 4096                    # elements of NaN pattern on each side of a guarded buffer
OUTSIDE = ("-2", "-1", "limit", "limit+1")


def outside(which: str, limit: int) -> int:
    """The planted value: two and one below the range [0, limit), the limit itself and one above it."""
    return {"-2": -2, "-1": -1, "limit": limit, "limit+1": limit + 1}[which]


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor as 16-bit words (every dtype of these tests is a multiple of 16 bits wide)."""
    return t.contiguous().view(torch.int16)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def is_pattern(t: torch.Tensor) -> bool:
    return bool((bits(t) == NAN16).all())


class Guarded:
    """A tensor inside a flat buffer with GUARD elements of a NaN pattern in front of and behind it."""

    def __init__(self, shape, dtype, dev, init=None):
        n = 1
        for s in shape:
            n *= s
        self.flat = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.fill_nan(self.flat)
        self.t = self.flat[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    @staticmethod
    def fill_nan(t):
        t.view(torch.int16).fill_(NAN16)

    @classmethod
    def of(cls, t: torch.Tensor):
        """A guarded copy of ``t`` (same bits)."""
        return cls(tuple(t.shape), t.dtype, t.device, init=t)

    def guards_intact(self):
        return is_pattern(self.flat[:GUARD]) and is_pattern(self.flat[-GUARD:])

    def bits(self):
        return bits(self.t)


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def tables(rot: int, n: int, dev):
    """The rotary sin / cos tables of ``n`` positions, each in a guarded buffer: a position outside [0, n) reads the guard."""
    from oracle.model import rotary_tables
    s, c = rotary_tables(rot, n)
    return Guarded.of(s.to(dev).contiguous()), Guarded.of(c.to(dev).contiguous())


class Operands:
    """The guarded operands of one launch by name, with a bitwise snapshot taken before it."""

    def __init__(self, **bufs):
        self.bufs = bufs
        self.before = {}

    def __getitem__(self, name):
        return self.bufs[name]

    def snapshot(self):
        self.before = {n: g.bits().clone() for n, g in self.bufs.items()}
        return self

    def expected(self, name):
        """A copy of operand ``name`` as it was before the launch, in the operand's dtype and shape: the test writes into it what
        the contract permits the launch to write."""
        g = self.bufs[name]
        return self.before[name].clone().view(g.t.dtype).view(g.t.shape)

    def check(self, what: str, **written):
        """(a) every guard band is intact; (b) every operand holds, bit for bit, what it held before the launch -- or ``written[name]``,
        the snapshot with the permitted writes applied."""
        torch.cuda.synchronize()
        for n, g in self.bufs.items():
            assert g.guards_intact(), f"{what}: a guard band of `{n}` was written"
        for n, g in self.bufs.items():
            want = bits(written[n]) if n in written else self.before[n]
            got = g.bits()
            if not torch.equal(got, want):
                bad = (got != want).reshape(g.t.shape[0], -1).any(1).nonzero().flatten().tolist()
                raise AssertionError(f"{what}: `{n}` differs from what the contract permits in rows {bad} of its first axis")


def assert_decode_attention(q, kcache, vcache, ctx_rows, what, out):
    """out [B, H * 256] of single-query attention over the first ctx_rows[b] keys of row b, per element against fp64 under the
    decode kernels' bound (kernel_compare.attention_bound with fp32 weights and one maximum, as test_kernels_gpu states it)."""
    import kernel_compare as kcmp
    heads = q.shape[1]
    worst = 0.0
    for b in range(q.shape[0]):
        c = int(ctx_rows[b])
        terms = kcmp.attention_terms(q[b], kcache[b, :, :c], vcache[b, :, :c])
        bound = kcmp.attention_bound(terms, c, out.dtype, p_dtype=torch.float32, n_rescale=0)
        worst = max(worst, kcmp.assert_elementwise(out[b].view(heads, 1, 256), terms["ref"], bound, f"{what}, row {b} (ctx {c})"))
    return worst
