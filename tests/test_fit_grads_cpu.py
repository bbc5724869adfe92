"""The float64 reference of one stage-1 fit step (tests/fit_grads_reference.py) against float64 autograd of the oracle
modules, the yardsticks its two comparators give at every shape of tests/test_gpu_fit_grads.py, and the conditions on
the seeded inputs that make those GPU cases meaningful.  CPU only."""
import numpy as np
import pytest
import torch

from tests import fit_grads_reference as R
from oracle.models import NeuralFeatureFieldOracle, SingleImageDenoiserOracle


def _small_case(seed=0):
    """C = 64, B = 64, 4 levels, 5 x 5 lattice, 3 views; natural (unshifted) biases."""
    cfg = R.Cfg(feat_dim=64, lattice=25, n_levels=4, log2_hashmap_size=8)
    feat, xy, idx = R.make_data(cfg, 64, 3, seed)
    rs = np.random.RandomState(seed)
    lay, n = R.layout(cfg)
    params = np.zeros(n, np.float32)
    for name, v in R.views(cfg, params).items():
        v[...] = rs.uniform(-0.3, 0.3, v.shape)
    return cfg, params, feat, xy, idx


@pytest.mark.parametrize("phase2", [False, True])
def test_reference_matches_float64_autograd(phase2):
    cfg, params, feat, xy, idx = _small_case()
    ref = R.reference(cfg, params, feat, xy, idx, phase2)
    pv = R.views(cfg, params)
    side = 5
    field = NeuralFeatureFieldOracle(feat_dim=cfg.feat_dim, base_resolution=cfg.base_resolution,
                                     max_resolution=cfg.max_resolution, n_levels=cfg.n_levels,
                                     log2_hashmap_size=cfg.log2_hashmap_size).double()
    den = SingleImageDenoiserOracle(side, side, cfg.feat_dim).double()
    with torch.no_grad():
        field.neural_field.params.copy_(torch.from_numpy(pv["grid"].reshape(-1)))
        for i, (w, b) in zip((0, 2), (("w1", "b1"), ("w2", "b2"))):
            field.mlp[i].weight.copy_(torch.from_numpy(pv[w]))
            field.mlp[i].bias.copy_(torch.from_numpy(pv[b]))
        den.shared_artifacts.copy_(torch.from_numpy(pv["G"]).view(1, side, side, cfg.feat_dim).permute(0, 3, 1, 2))
        for i, (w, b) in zip((0, 2, 4), (("wh1", "bh1"), ("wh2", "bh2"), ("wh3", "bh3"))):
            den.residual_predictor[i].weight.copy_(torch.from_numpy(pv[w]))
            den.residual_predictor[i].bias.copy_(torch.from_numpy(pv[b]))
    if phase2:
        den.stop_shared_artifacts_grad()
        den.start_residual_predictor()
    lin = torch.linspace(-1, 1, side, dtype=torch.float64)  # the lattice points of G, in float64
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    sa = torch.stack([gx, gy], -1).reshape(-1, 2)
    ridx = torch.from_numpy(idx.astype(np.int64))
    out = den(raw_vit_outputs=torch.from_numpy(feat).double()[ridx], global_pixel_coords=torch.from_numpy(xy)[ridx],
              neural_field=field, shared_artifact_coords=sa[ridx % cfg.lattice])
    (out["loss"] * cfg.grad_scale).backward()
    got = {"grid": field.neural_field.params.grad.view(-1, cfg.n_features),
           "w1": field.mlp[0].weight.grad, "b1": field.mlp[0].bias.grad,
           "w2": field.mlp[2].weight.grad, "b2": field.mlp[2].bias.grad}
    if phase2:
        assert den.shared_artifacts.grad is None and "G" not in ref["g"]
        for i, (w, b) in zip((0, 2, 4), (("wh1", "bh1"), ("wh2", "bh2"), ("wh3", "bh3"))):
            got[w], got[b] = den.residual_predictor[i].weight.grad, den.residual_predictor[i].bias.grad
    else:
        assert all(p.grad is None for p in den.residual_predictor.parameters()) and "wh1" not in ref["g"]
        got["G"] = den.shared_artifacts.grad.permute(0, 2, 3, 1).reshape(cfg.lattice, cfg.feat_dim)
    assert sorted(got) == sorted(ref["g"])
    for name, g in got.items():
        a, b = g.numpy(), ref["g"][name]
        rel = np.abs(a - b).max() / np.abs(a).max()
        assert rel < 1e-12, (name, rel)
        # the magnitude bounds the element, and is attained where all terms share a sign
        assert (np.abs(b) <= ref["mag"][name] * (1 + 1e-12) + 1e-300).all(), name
    for key, want in zip(R.LOSS_KEYS, ref["loss"]):
        have = float(out[key]) if key in out else 0.0
        assert abs(have - want) <= 1e-12 * max(1.0, abs(have)), (key, have, want)


@pytest.mark.parametrize("C", sorted(R.SHAPES))
def test_yardsticks_and_input_conditions(C):
    """Both comparators against the reference at every GPU shape (printed: these are the yardsticks the GPU cases use), and
    the input conditions for every fit of the shape."""
    B, side, V = R.SHAPES[C]
    for fit in range(R.N_FITS):
        cfg, params, feat, xy, idx, seed = R.case(C, fit)
        assert R.input_conditions(cfg, params, feat, xy, idx) == [], (C, fit, seed)
        assert len(idx) == B and feat.shape == (V * side * side, C)
    for bf16 in (False, True):
        for phase2 in (False, True):
            ref, want, yard, (loss_l2, loss_max) = R.yardstick(C, 0, bf16, phase2)
            print(f"C={C} {'bf16' if bf16 else 'fp32'} phase {2 if phase2 else 1}: loss L2 {loss_l2:.2e} max {loss_max:.1f} u")
            for label, (l2, mx) in yard.items():
                print(f"    {label:12s} rel L2 {l2:.3e}   max err {mx:.3g} u*scale")
                bound = 2e-6 if not bf16 else 8e-2  # a few hundred u / a few bf16 roundings (2^-9 each) along the chain
                assert 0.0 < l2 < bound, (label, l2)
            # alignment padding has zero scale and zero gradient
            for label, (w, s) in want.items():
                assert (w[s == 0] == 0).all()
    # the comparators round where they say they do: bf16 lands ~2^-9 from float64, fp32 ~2^-24
    y32, y16 = R.yardstick(C, 0, False, False)[2], R.yardstick(C, 0, True, False)[2]
    assert y16["w2"][0] > 100 * y32["w2"][0]
