"""tests/muon_ref.py, the fp64 reference of FlatAdam's orthogonalised-momentum step, against torch.optim.Muon on the CPU.

torch runs the Newton-Schulz iteration in bf16, so single elements do not agree (the largest element deviation after three steps is
0.15 - 0.3 of a step's rms).  What is compared is the displacement D = w3 - w0 over three steps with weight decay 0.1:
||D_torch - D_ref||_F / ||D_ref||_F.  Measured on the CPU (torch 2.10), shape x adjust_lr_fn:

    (64, 384)  original 0.0106  match_rms_adamw 0.0107
    (768, 32)  original 0.0174  match_rms_adamw 0.0174
    (87, 200)  original 0.0099  match_rms_adamw 0.0100
    (4, 32)    original 0.0132  match_rms_adamw 0.0132

The bound is twice the largest, 0.035 (far below the 0.2 at which the reference would be wrong).  A reference with the other scale rule
(measured 0.11 - 2.9), without the Nesterov term (0.20 - 0.24) or with m = mu m + g (0.19 - 0.23) must exceed it on every case."""
import numpy as np
import pytest
import torch

from tests import muon_ref as R

BOUND = 0.035
SHAPES = [(64, 384), (768, 32), (87, 200), (4, 32)]
MODES = ["original", "match_rms_adamw"]
LR, WD, MU = 0.02, 0.1, 0.95


def _case(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn(shape, generator=g) * 0.05
    grads = [torch.randn(shape, generator=g) for _ in range(3)]
    return w0, grads


_TORCH = {}


def _torch_displacement(shape, mode):
    """computed once per case and shared by the four tests that compare against it"""
    key = (shape, mode)
    if key not in _TORCH:
        w0, grads = _case(shape)
        p = torch.nn.Parameter(w0.clone())
        opt = torch.optim.Muon([p], lr=LR, weight_decay=WD, momentum=MU, nesterov=True, adjust_lr_fn=mode)
        for g in grads:
            p.grad = g.clone()
            opt.step()
        _TORCH[key] = (p.detach() - w0).numpy().astype(np.float64)
    return _TORCH[key]


def _ref_displacement(shape, mode, variant=None):
    """three steps by the reference, the state carried in fp32 as an optimizer does; `variant` plants one mistake"""
    w0, grads = _case(shape)
    w, m = w0.numpy().copy(), np.zeros(shape, np.float32)
    for g in grads:
        g = g.numpy()
        if variant == "m_plus_g":                         # m = mu m + g, the rest by the rule
            m1 = MU * m.astype(np.float64) + g.astype(np.float64)
            u = (1.0 - MU) * g.astype(np.float64) + MU * m1
            O = R.ns(u.astype(np.float32)).astype(np.float64)
            w1 = w.astype(np.float64) * (1.0 - LR * WD) - LR * R.scale_of(shape[0], shape[1], mode) * O
            w, m = w1.astype(np.float32), m1.astype(np.float32)
            continue
        kw = dict(lr=LR, wd=WD, mu=MU, nesterov=variant != "no_nesterov", scale=mode, decoupled=True)
        if variant == "other_scale":
            kw["scale"] = MODES[1 - MODES.index(mode)]
        out = R.step(w, m, g, **kw)
        w, m = out["w"].astype(np.float32), out["m"].astype(np.float32)
    return w.astype(np.float64) - w0.numpy().astype(np.float64)


def _rel(shape, mode, variant=None):
    dt, dr = _torch_displacement(shape, mode), _ref_displacement(shape, mode, variant)
    return float(np.linalg.norm(dt - dr) / np.linalg.norm(dr))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_follows_torch_muon(shape, mode):
    rel = _rel(shape, mode)
    print(f"{shape} {mode}: {rel:.4f}")
    assert rel < BOUND


@pytest.mark.parametrize("variant", ["other_scale", "no_nesterov", "m_plus_g"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_planted_mistake_exceeds_the_bound(shape, mode, variant):
    rel = _rel(shape, mode, variant)
    print(f"{shape} {mode} {variant}: {rel:.4f}")
    assert rel > BOUND


BAND_SHAPES = [(4, 32), (16, 64), (32, 128), (87, 400), (768, 32), (128, 1000), (96, 1536), (8, 32), (64, 384), (3, 12)]      # aspect >= 4


def test_singular_values_of_the_iteration():
    """five iterations do not orthogonalise exactly: they bring the singular values of a Gaussian matrix of aspect >= 4 into
    [0.6, 1.25] (measured in fp64 over these shapes: [0.68, 1.21]) and keep those of ANY input at or below 1.25"""
    rng = np.random.default_rng(0)
    for rows, cols in BAND_SHAPES:
        for kind in ("gauss", "lowrank", "rowscale"):
            sv = np.linalg.svd(R.ns(R.inputs(kind, rows, cols, rng)), compute_uv=False)
            assert sv.max() <= 1.25, (rows, cols, kind, sv.max())
            if kind == "gauss":
                assert sv.min() >= 0.6, (rows, cols, sv.min())


def test_zeros_stay_zeros_and_orientation():
    assert not R.ns(np.zeros((5, 9), np.float32)).any()
    rng = np.random.default_rng(1)
    g = R.inputs("gauss", 7, 40, rng)
    np.testing.assert_allclose(R.ns(g.T), R.ns(g).T, rtol=0, atol=1e-12)        # the tall orientation is the transpose of the wide one
    o64, tol = R.ns_tolerance(g)
    assert tol < 1e-3 * R.rms(o64)                                               # the fp32 yardstick stays far below the signal
