"""MagmaEngine._train_block_kind on fakes of the fields it reads: pure host logic, no GPU.  The thirteen configurations of
tests/launch_trace.py TRAIN_CASES; a block without an MLP adapter (whose ``blk.mlp`` is the bare MLP and cannot be subscripted) once
crashed the training step."""
from types import SimpleNamespace as NS

import pytest

from magma_amd.train_engine import BlockKind, MagmaEngine

SWITCHES = dict(fp8=False, fp8_attn=True, fp8_mx=True, fp8_adapters=True, cat_up=True, lm_trainable=False)
FP8 = dict(fp8=True)


def adapter(d, r, plain=True):
    return NS(plain=plain, down=NS(weight=NS(shape=(r, d))), up=NS(weight=NS(shape=(d, r))))


def block(mlp=None, attn=None, d=512, r=128, plain=True, out_bias=None):
    """(layer fields, block module): mlp / attn in (None, "serial", "parallel")."""
    ly = NS(mlp_adapter=None if mlp is None else object(), mlp_par=object() if mlp == "parallel" else None,
            attn_adapter=None if attn is None else object(), attn_par=object() if attn == "parallel" else None,
            _src=(NS(out_proj=NS(bias=out_bias)), object()))
    # Sequential(mlp, Adapter) only for a serial adapter; anything else must never be subscripted
    return ly, NS(mlp=[object(), adapter(d, r, plain)] if mlp == "serial" else object(), attn=object())


def engine(blk, **switches):
    eng = MagmaEngine.__new__(MagmaEngine)
    for k, v in {**SWITCHES, **switches}.items():
        setattr(eng, k, v)
    eng.module = NS(lm=NS(engine=NS(layers=[blk[0]]), transformer=NS(h=[blk[1]])))
    return eng


CASES = {
    "v1": (block("serial"), {}, ("cat", "none", "rows")),
    "v1_nocat": (block("serial"), dict(cat_up=False), ("serial", "none", "rows")),
    "v1_allrows": (block("serial"), {}, ("cat", "none", "rows")),
    "v1_recompute": (block("serial"), {}, ("cat", "none", "rows")),
    "v2": (block("serial", "serial", r=64), {}, ("serial", "serial", "rows")),
    "attn_only": (block(None, "serial"), {}, ("none", "serial", "rows")),
    "no_adapters": (block(), {}, ("none", "none", "rows")),
    "parallel": (block("parallel", "parallel"), {}, ("parallel", "parallel", "rows")),
    "ln_gelu_erf": (block("serial", plain=False), {}, ("serial", "none", "rows")),
    "lm_trainable": (block("serial"), dict(lm_trainable=True), ("serial", "none", "rows")),
    "fp8_row": (block("serial"), dict(FP8, fp8_attn=False, fp8_mx=False), ("serial", "none", "rows")),
    "fp8_mx": (block("serial"), dict(FP8, fp8_adapters=False), ("serial", "none", "fp8")),
    "fp8_all": (block("serial", r=256), FP8, ("fp8", "none", "fp8")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kind_of_the_thirteen_configurations(name):
    blk, switches, want = CASES[name]
    assert engine(blk, **switches)._train_block_kind(0) == BlockKind(*want)


def test_conditions_at_their_edges():
    kind = lambda blk, **sw: tuple(engine(blk, **sw)._train_block_kind(0))  # noqa: E731
    assert kind(block("serial", r=128), **FP8)[0] == "serial"                         # r % 256: the MX output does not cover it
    assert kind(block("serial", r=256, plain=False), **FP8)[0] == "serial"
    assert kind(block("parallel", r=256), **FP8) == ("parallel", "none", "fp8")       # parallel before fp8
    assert kind(block("serial", out_bias=object()))[0] == "serial"                    # [W_out | W_up] carries b_up only
    assert kind(block("serial", r=132))[0] == "serial"                                # 16-byte aligned [:, d:] view
    assert kind(block("serial", "parallel"))[:2] == ("serial", "parallel")            # no cat beside an attention adapter
    assert kind(block("serial"), fp8=True, fp8_attn=False)[0] == "serial"             # cat is the bf16 step's
    for sw in (dict(FP8), dict(FP8, fp8_mx=False), dict(lm_trainable=True), dict(cat_up=False)):
        assert kind(block(), **sw)[:2] == ("none", "none") and kind(block(None, "parallel"), **sw)[:2] == ("none", "parallel")
