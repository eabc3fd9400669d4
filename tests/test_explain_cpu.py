"""Explaining an answer, the host side (DESIGN.md "Explaining an answer"): the scale vectors of the similarity rule, the units, the
work list, Explanation.grid -- and the CPU statement the GPU tests compare against, which at scale 1 is oracle.model.lm_forward."""
import pytest
import torch

from magma_amd.sampling import (Explanation, check_explain_args, explain_units, explain_work_list, mean_nll, unit_scale)


# --------------------------------------------------------------------------------------------------------------------- (l)
def planted():
    """Positions 0 and 1: exact duplicates; 2: cosine 0.8 with them; 3: orthogonal to all."""
    e = torch.zeros(4, 8)
    e[0, 0] = e[1, 0] = 2.0
    e[2, 0], e[2, 1] = 0.8 * 3, 0.6 * 3
    e[3, 2] = 5.0
    return e


def test_similarity_rule_on_planted_embeddings():
    e, s, kappa = planted(), 0.9, 0.7
    one = torch.tensor(1.0)
    got = unit_scale(e, [0], s, kappa)
    assert got.dtype == torch.float32 and got.shape == (4,)
    assert got[0] == one - s and got[1] == one - s           # the duplicate of the unit's position: c = 1
    assert abs(float(got[2]) - (1 - 0.8 * s)) < 1e-6         # the 0.8 neighbour
    assert got[3] == 1.0                                     # the orthogonal one
    # kappa above 0.8: the neighbour is left alone, the duplicate is not
    got = unit_scale(e, [0], s, 0.85)
    assert got.tolist() == [float(one - s), float(one - s), 1.0, 1.0]
    # a unit of several positions takes the largest cosine; the unit's own positions have c = 1 whatever their embeddings
    got = unit_scale(e, [2, 3], s, kappa)
    assert got[2] == one - s and got[3] == one - s
    assert abs(float(got[0]) - (1 - 0.8 * s)) < 1e-6 and abs(float(got[1]) - (1 - 0.8 * s)) < 1e-6
    # a zero embedding has no direction: cosine 0, never similar
    z = planted()
    z[3] = 0
    assert unit_scale(z, [0], s, kappa)[3] == 1.0 and unit_scale(z, [3], s, kappa).tolist() == [1.0, 1.0, 1.0, float(one - s)]


def test_scale_vector_without_a_threshold():
    e = planted()
    assert unit_scale(e, [1, 3], 0.75).tolist() == [1.0, 0.25, 1.0, 0.25]
    assert unit_scale(e, [2], 0.0).tolist() == [1.0] * 4
    assert unit_scale(e.to(torch.bfloat16), [0], 1.0, 0.7).tolist()[:2] == [0.0, 0.0]
    assert bool((unit_scale(e, [0], 1.0, -1.0) >= 0).all())


# ------------------------------------------------------------------------------------------------------ units and work list
def test_units():
    assert explain_units([2, 3]) == [[[0], [1]], [[0], [1], [2]]]
    assert explain_units(torch.tensor([2, 3]), [[[1, 0]], [torch.tensor([2]), (0, 1)]]) == [[[1, 0]], [[2], [0, 1]]]
    for bad in ([[[2]], [[0]]], [[[0]], [[3]]], [[[-1]], [[0]]], [[[]], [[0]]], [[[0]]]):
        with pytest.raises(ValueError):
            explain_units([2, 3], bad)


def test_work_list_has_one_shape_per_forward():
    work = explain_work_list([2, 0, 3], 4)
    assert work == [(0, -1), (0, 0), (0, 1), (1, -1), (2, -1), (2, 0), (2, 1), (2, 2)]
    work = explain_work_list([2, 3], 4)
    assert len(work) == 8 and work[:7] == [(0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (1, 2)] and work[7] == (0, -1)
    assert len(explain_work_list([5], 16)) == 16 and explain_work_list([5], 1) == [(0, u) for u in range(-1, 5)]


def test_scalar_arguments():
    check_explain_args(0.0, None, 1)
    check_explain_args(1, 0.5, 64)
    for bad in (dict(suppression=-0.1), dict(suppression=1.01), dict(suppression=float("nan")), dict(suppression=None),
                dict(similarity_threshold=float("inf")), dict(similarity_threshold="0.7"), dict(batch_size=0),
                dict(batch_size=-3), dict(batch_size=2.0), dict(batch_size=True)):
        with pytest.raises(ValueError):
            check_explain_args(**bad)


def test_mean_nll():
    lp = torch.tensor([[-1.0, -2.0, 0.0], [-3.0, -3.0, -3.0]])
    assert mean_nll(lp, torch.tensor([2, 3])).tolist() == [1.5, 3.0]


# --------------------------------------------------------------------------------------------------------------------- (n)
def test_grid_is_the_stated_view():
    rel = torch.arange(2 * 20, dtype=torch.float32).view(2, 20)
    ex = Explanation(rel, torch.zeros(2), rel.clone(), torch.tensor([20, 20]))
    g = ex.grid(1, 3, 4, 3)
    assert g.shape == (4, 3) and torch.equal(g, rel[1, 3:15].view(4, 3))
    assert g.data_ptr() == rel[1, 3:].data_ptr()              # a view, not a copy
    assert torch.equal(ex.grid(0, 0, 1, 20), rel[0:1])
    for bad in ((0, 10, 4, 3), (0, -1, 2, 2), (0, 0, 0, 3)):
        with pytest.raises(ValueError):
            ex.grid(*bad)


# ------------------------------------------------------------------------------------------------------- the CPU statement
def test_statement_at_scale_one_is_the_oracle():
    from oracle.model import OracleConfig, attn_prefix, init_params, lm_forward
    from test_explain_gpu import lm_forward_scaled
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=0)
    params = init_params(cfg, seed=11)
    for i in range(cfg.n_layer):
        for w in ("q_proj.weight", "k_proj.weight"):
            params[attn_prefix(cfg, i) + w] = params[attn_prefix(cfg, i) + w] * 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, cfg.d_model, generator=g)
    for dtype in (torch.float32, torch.bfloat16):
        p = {k: v.to(dtype) for k, v in params.items()}
        want = lm_forward(p, cfg, inputs_embeds=x.to(dtype))["logits"]
        assert torch.equal(lm_forward_scaled(p, cfg, x.to(dtype), torch.ones(2, 7)), want)
    ks = torch.ones(2, 7)
    ks[0, 2] = 0.1
    got = lm_forward_scaled(params, cfg, x, ks)
    want = lm_forward(params, cfg, inputs_embeds=x)["logits"]
    assert torch.equal(got[1], want[1]) and torch.equal(got[0, :2], want[0, :2])      # causal: rows before the key are untouched
    assert not torch.equal(got[0, 2:], want[0, 2:])
