"""tests/bn_cases.py checked on the CPU: no kernel is called here.

1. The inputs are fit for the acceptance rule of tests/test_conv_bn_units_gpu.py (rel-L2 e <= 2 e_bf16 + 1e-2 per trunk tensor).
   Frozen statistics: in every family the fp64 oracle's gradient of every trunk tensor is non-zero -- or a structural zero behind a
   gain of exactly zero, which the bf16 oracle reproduces exactly -- and the bf16 oracle stays below 0.1 of it, so the rule bounds
   every tensor at 0.21 and an error of order 1 cannot pass.  Batch statistics: the whole-trunk yardstick is unusable (comment in
   the test); 4 takes its place.
2. The rule can tell the two ways of forming dgamma apart before it runs on a GPU: an fp32 stand-in of one unit's backward that
   takes x-hat from the rounded output FAILS it in small_gain, clip_init and zero_some and passes in benign; the one that takes
   x-hat from z (through <W, g^T a>) passes in every family.
3. A correct implementation CAN pass on the chosen draws: the whole trunk in the engine's units on the host
   (bn_cases.trunk_standin) satisfies the rule for every tensor of every family, with bn_cases.SEED_MARGIN to spare.
4. Batch statistics, unit by unit: autograd through ONE conv -> BatchNorm(batch statistics) in bf16 is a fit yardstick for every
   tensor of every unit of every family (`offset` included), except where gains of 1e-2 make a unit ill-conditioned for any bf16 z."""
import pytest
import torch

import bn_cases as bc

CASES = [(f, False) for f in bc.FROZEN_FAMILIES] + [(f, True) for f in bc.FAMILIES]


@pytest.mark.parametrize("family,bn_train", CASES, ids=[f"{f}-{'batch' if b else 'frozen'}" for f, b in CASES])
def test_reference_is_fit_for_the_acceptance_rule(family, bn_train):
    ref = bc.reference(family, bn_train)
    g64, g_bf = ref["g64"], ref["g_bf"]
    assert len(g64) == 3 * 22           # 22 conv+BatchNorm units in the (1, 1, 2, 1) trunk: weight, gain, shift each
    worst, zeros = [], []
    for n, r in g64.items():
        if float(r.norm()) == 0.0:
            zeros.append(n)
            assert float(g_bf[n].double().norm()) == 0.0, f"{n}: fp64 gradient is exactly zero, the bf16 oracle's is not"
            continue
        worst.append((bc.rel_l2(g_bf[n], r), n))
    worst.sort(reverse=True)
    print(f"[bn_cases] {family} {'batch' if bn_train else 'frozen'}: worst bf16-oracle errors",
          [(n[len(bc.ENC):], f"{e:.2e}") for e, n in worst[:5]], f"; {len(zeros)} structural zeros")
    # structural zeros: only behind the zero bn3 gains of clip_init (conv1..3, bn1, bn2 of each of the five bottlenecks)
    if family == "clip_init":
        assert len(zeros) == 5 * 7 and all(".bn3." not in n and "downsample" not in n and "layer" in n for n in zeros), zeros
    else:
        assert not zeros, zeros
    assert float(ref["feats64"].abs().max()) > 0 and all(bool(torch.isfinite(g).all()) for g in g_bf.values())
    if bn_train:
        # Batch statistics: the condition cannot be met by ANY constants at this trunk, the control included, nor by more rows per
        # channel (benign at 2 / 8 / 16 images of 64 x 64 and 4 of 128 x 128: median e_bf16 0.32 / 0.28 / 0.30 / 0.29).  The bf16
        # oracle's forward error grows by about 1.2 x per unit under re-normalisation (0.3 % after the stem, 4 - 11 % at the output;
        # 0.4 % throughout with frozen statistics) and on the committed draws its worst per-tensor gradient error is 1.11 (benign),
        # 0.85 (trained), 0.22 (clip_init), 0.70 (zero_some), 0.88 (offset); in small_gain the outputs are beta + 1e-2 x-hat, whole
        # channels have one ReLU gate, a batch BatchNorm behind them cancels a shift exactly, and some shift gradients are rounding
        # noise in fp64 (e_bf16 4e12).  So the whole-trunk per-tensor rule DECIDES NOTHING in this mode: it admits errors of order 1.
        # What decides is the unit-level comparison (test_unit_level_yardstick_is_fit_under_batch_statistics below; the GPU
        # test's check_units_against_the_layer), whose yardstick condition is asserted.
        return
    assert worst[0][0] < 0.1, worst[:5]


def test_offset_family_shifts_the_stem_channels():
    """|mean| / std of the first convolution's output, per channel: the median of 10 |N(0, 1)| is 6.7."""
    import torch.nn.functional as F
    cfg, p = bc.trunk_params("offset")
    z = F.conv2d(bc.images_for("offset").double(), p[bc.ENC + "conv1.weight"].double(), None, stride=2, padding=1)
    ratio = (z.mean((0, 2, 3)).abs() / z.std((0, 2, 3)))
    print("[bn_cases] offset: |mean| / std of the stem channels", [f"{float(v):.1f}" for v in ratio])
    assert float(ratio.median()) > 3.0 and float(ratio.max()) > 10.0


def test_zero_gains_are_signed_zeros_on_every_fourth_channel():
    _, p = bc.trunk_params("zero_some")
    masks = bc.zero_gain_channels(p)
    assert len(masks) == 22
    for n, m in masks.items():
        assert m.nonzero().flatten().tolist() == list(range(0, m.numel(), 4)), n
        signs = torch.signbit(p[n][m]).tolist()
        assert signs == [i % 2 == 1 for i in range(len(signs))], n          # +0.0, -0.0 in turn
    _, p = bc.trunk_params("clip_init")
    masks = bc.zero_gain_channels(p)
    assert sorted(masks) == sorted(k for k in p if ".bn3.weight" in k and "layer" in k) and all(bool(m.all()) for m in masks.values())


@pytest.mark.parametrize("family", bc.FROZEN_FAMILIES)
def test_rule_separates_xhat_from_output_and_xhat_from_z(family):
    c = bc.unit_case(family)
    ref, bf = bc.unit_autograd(c, torch.float64), bc.unit_autograd(c, bc.BF16)
    verdict, zero = {}, c["gamma"] == 0
    for form in ("y", "z"):
        got = bc.unit_standin(c, form)
        for k in ("dW", "dgamma", "dbeta"):
            ok, e, e_bf = bc.acceptable(got[k], bf[k], ref[k])
            if k == "dgamma" and bool(zero.any()):         # the rule's second clause: the zero-gain channels on their own
                ok_z, e_z, e_bf_z = bc.acceptable(got[k][zero], bf[k][zero], ref[k][zero])
                print(f"[bn_cases] unit {family}: x-hat from {form}: dgamma on the zero-gain channels e {e_z:.3e} e_bf16 {e_bf_z:.3e}")
                ok = ok and ok_z
            verdict[form, k] = ok
            print(f"[bn_cases] unit {family}: x-hat from {form}: {k} e {e:.3e} e_bf16 {e_bf:.3e} {'ok' if ok else 'FAILS the rule'}")
    assert float(ref["dgamma"].norm()) > 0 and float(ref["dbeta"].norm()) > 0
    # x-hat from z: every tensor passes in every family
    assert all(verdict["z", k] for k in ("dW", "dgamma", "dbeta")), verdict
    # the weight and shift gradients never depended on x-hat
    assert verdict["y", "dW"] and verdict["y", "dbeta"], verdict
    if family in bc.HARD_FAMILIES:
        assert not verdict["y", "dgamma"], "the rule accepts x-hat taken from the rounded output: the GPU test could not see the defect"
    if family == "benign":
        assert verdict["y", "dgamma"]
    # the channels whose gain is exactly zero: the output holds nothing about z there
    if bool(zero.any()):
        assert float(ref["dgamma"][zero].norm()) > 0
        assert float(bc.unit_standin(c, "y")["dgamma"][zero].abs().max()) == 0.0
        ok, e, e_bf = bc.acceptable(bc.unit_standin(c, "z")["dgamma"][zero], bf["dgamma"][zero], ref["dgamma"][zero])
        assert ok, (e, e_bf)


@pytest.mark.parametrize("family", bc.FROZEN_FAMILIES)
def test_an_honest_second_implementation_passes_on_the_chosen_draws(family):
    ref = bc.reference(family, False)
    feats, grads = bc.trunk_standin(ref["cfg"], ref["params"], ref["images"], ref["R"])
    excess = bc.rule_excess(grads, ref["g_bf"], ref["g64"], ref["params"])
    print(f"[bn_cases] {family}: trunk stand-in, worst e - (2 e_bf16 + 1e-2) = {excess:.4f}; feats rel-L2 {bc.rel_l2(feats, ref['feats64']):.2e} "
          f"(bf16 oracle {bc.rel_l2(ref['feats_bf'], ref['feats64']):.2e})")
    assert excess <= -bc.SEED_MARGIN, excess
    for n, mask in bc.zero_gain_channels(ref["params"]).items():
        ok, e, e_bf = bc.acceptable(grads[n][mask], ref["g_bf"][n][mask], ref["g64"][n][mask])
        assert ok and (float(ref["g64"][n][mask].norm()) == 0 or float(grads[n][mask].abs().max()) > 0), (n, e, e_bf)


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_unit_level_yardstick_is_fit_under_batch_statistics(family):
    """The whole-trunk yardstick is unusable under batch statistics (above); the unit-level one is not: for every unit, on operands
    taken from the fp64 oracle, autograd through conv -> BatchNorm(batch statistics) in bf16 is a fit yardstick (bn_cases.unit_yardstick: below 0.1; below 0.25 where a batch mean lies more than 8 deviations from zero, as in
    `offset`'s stem) for the weight, gain and shift gradient, so the rule bounds each at 0.21 (0.51), and a dgamma that is zero fails it."""
    units = bc.oracle_unit_operands(family)
    assert len(units) == 22
    worst, unfit = [], []
    for name, kind, a, geom, w, gamma, beta, g in units:
        r64 = bc.unit_layer_grads(kind, a, geom, w, gamma, beta, g, torch.float64)
        rbf = bc.unit_layer_grads(kind, a, geom, w, gamma, beta, g, bc.BF16)
        kappa = r64["kappa"]
        for k in ("dW", "dgamma", "dbeta"):
            r = r64[k]
            if float(r.norm()) == 0.0:          # no incoming gradient, or a weight behind a gain of exactly zero
                assert float(rbf[k].norm()) == 0.0, (name, k)
                continue
            e_bf = bc.rel_l2(rbf[k], r)
            if bc.unit_yardstick(e_bf, kappa) == "unfit":
                unfit.append((name + " " + k, f"{e_bf:.2e}", f"kappa {kappa:.0f}"))
                continue
            worst.append((e_bf, name + " " + k, kappa))
            if k == "dgamma":                     # what the check must reject: no gain gradient at all
                ok, e, _ = bc.acceptable(torch.zeros_like(r), rbf[k], r)
                assert not ok, (name, e, e_bf)
    worst.sort(reverse=True)
    print(f"[bn_cases] {family} batch, unit by unit: worst bf16 errors", [(n, f"{e:.2e}", f"kappa {kp:.1f}") for e, n, kp in worst[:4]],
          f"; unfit: {unfit}")
    # unfit tensors: only where gains of 1e-2 make a unit's input nearly constant per channel (means hundreds of deviations
    # from zero: a z held in bf16 cannot carry such a unit, in the oracle or in the engine); in every other family every tensor of
    # every unit is held to the rule
    assert not unfit or family == "small_gain", unfit
