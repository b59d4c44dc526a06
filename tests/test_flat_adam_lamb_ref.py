"""The fp64 checker of the trust-ratio step (tests/lamb_ref.py) against an emulation of the device's arithmetic with correctly rounded
fp32 operations on the host: the checker accepts the emulated step of every kind of range the GPU test uses, and refuses a step that is
off by what the bounds are there to catch.  No GPU."""
import numpy as np
import pytest
import torch

from tests import lamb_ref

B1, B2, EPS, LR, WD = np.float32(0.9), np.float32(0.999), np.float32(1e-8), np.float32(3e-3), np.float32(1e-2)
CLIP = 2.0


def corrections(n):
    return np.float32(1.0 - float(B1) ** n), np.float32(np.sqrt(1.0 - float(B2) ** n))


def run(shape, scale, decoupled, adapted, steps=4, zero_grad=False, wd=WD, seed=0):
    """-> the arguments of check_range for the last of `steps` emulated steps"""
    g = np.random.default_rng(seed)
    p = (g.standard_normal(shape) * scale).astype(np.float32).reshape(-1)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for k in range(steps):
        grad = np.zeros_like(p) if zero_grad else g.standard_normal(p.shape).astype(np.float32)
        bc1, bc2 = corrections(k + 1)
        p0 = p
        p, m, v, wn, un, ratio = lamb_ref.emulate_step(p0, grad, m, v, LR, np.float32(0.55), wd, B1, B2, EPS, bc1, bc2, np.float32(0.07), decoupled,
                                                       adapted, CLIP)
    t = torch.from_numpy
    return dict(p0=t(p0), p1=t(p), m1=t(m), v1=t(v), w_norm=wn, u_norm=un, ratio=ratio, lr=float(LR), lr_factor=0.55, wd=float(wd),
                bc1=float(bc1), bc2_sqrt=float(bc2), eps=float(EPS), decoupled=decoupled, adapted=adapted, clip=lamb_ref.f32(CLIP))


CASES = {"free": dict(shape=(260, 257), scale=0.5, adapted=True), "clamped": dict(shape=(3, 683), scale=4.0, adapted=True),
         "off": dict(shape=(1024,), scale=1.0, adapted=False), "zero_w": dict(shape=(3, 5), scale=0.0, adapted=True, steps=1),
         "zero_u": dict(shape=(1, 5), scale=1.0, adapted=True, zero_grad=True, wd=np.float32(0.0))}


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_checker_accepts_the_emulated_step(case, decoupled):
    args = run(decoupled=decoupled, **CASES[case])
    used, got = lamb_ref.check_range(**args)
    assert got == case
    assert used["p"] <= 0.6 and used["u_norm"] <= 0.6 and (used["ratio"] is None or used["ratio"] <= 0.6), used
    if case in ("off", "zero_w", "zero_u"):
        assert args["ratio"] == 1.0
    if case == "clamped":
        assert args["ratio"] == CLIP


def test_the_checker_refuses_what_the_bounds_are_there_to_catch():
    good = run(decoupled=True, **CASES["free"])
    lamb_ref.check_range(**good)
    # one element of p moved by 16 ulp
    bad = dict(good, p1=good["p1"].clone())
    bad["p1"][1234] = torch.nextafter(bad["p1"][1234], torch.tensor(np.inf)).item() + 16 * float(np.spacing(np.float32(abs(bad["p1"][1234].item()))))
    with pytest.raises(AssertionError, match="'p'"):
        lamb_ref.check_range(**bad)
    # a ratio off by 1e-5 relative: the parameters were updated with another word than the report's
    with pytest.raises(AssertionError, match="ratio"):
        lamb_ref.check_range(**dict(good, ratio=lamb_ref.f32(good["ratio"] * (1 + 1e-5))))
    # a norm off by 4 ulp / 1e-5 relative
    with pytest.raises(AssertionError, match="w_norm"):
        lamb_ref.check_range(**dict(good, w_norm=lamb_ref.f32(good["w_norm"] * (1 + 4 * 2.0 ** -23))))
    with pytest.raises(AssertionError, match="u_norm"):
        lamb_ref.check_range(**dict(good, u_norm=lamb_ref.f32(good["u_norm"] * (1 + 1e-5))))
    # the decay term left out of the update direction (coupled arithmetic under decoupled decay)
    with pytest.raises(AssertionError):
        lamb_ref.check_range(**dict(good, decoupled=False))
    # a range that is not adapted, a zero-norm one and a clamped one must report exactly 1 / the clamp
    off = run(decoupled=True, **CASES["off"])
    with pytest.raises(AssertionError, match="not adapted"):
        lamb_ref.check_range(**dict(off, ratio=lamb_ref.f32(1.0 + 2.0 ** -23)))
    clamped = run(decoupled=False, **CASES["clamped"])
    with pytest.raises(AssertionError, match="clamp"):
        lamb_ref.check_range(**dict(clamped, ratio=lamb_ref.f32(CLIP * (1 + 2.0 ** -23))))
