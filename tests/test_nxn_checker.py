"""What the element-wise fp64 check of the N x N strip kernels (tests/nxn_ref.py, used on the GPU by tests/test_nxn_strips_fp64_gpu.py)
catches, shown on the CPU: each op of avmoe_nxn_strip is emulated in torch with the kernel's roundings (bf16 operands, fp32 products and
exponentials, att and dS rounded to bf16 before the second product, fp32 read-modify-write, bf16 store) --

  * the honest emulation stays inside the bound at every shape and input family of the GPU test (the worst ratios are printed), and
  * each mutation a strip kernel could plausibly suffer is REJECTED, for every op that has the operand: one 128-token streamed tile left
    out of the contraction (first, middle, last), the log-sum-exp of the row 16 below (the `tm` halves swapped), the row dot of the
    neighbouring row, frame f computed with frame f - 1's log-sum-exp, DXQ and DXK exchanged, the running sum not rescaled when a later
    tile raises the maximum, `out` overwritten instead of accumulated.

`att` NOT rounded to bf16 before the second product is deliberately NOT a failure: the rounding is an allowance of the bound (the kernels
keep it to reproduce the stored softmax they replaced), not something a reference in fp64 can demand."""
import pytest
import torch

from tests import nxn_ref as R

RATIOS = {}


def rb(t):
    return t.bfloat16().float()


def _halves_swapped(v):
    """row r of a wave's 32 rows <-> row r + 16 (the two `tm` fragments of nxn_att.hip)"""
    F, N = v.shape
    return v.reshape(F, N // 32, 2, 16).flip(2).reshape(F, N)


def emulate(op, X, dxr=None, lse=None, rowdot=None, out0=None, att_in=None, mut=None, drop=None):
    """One op with the kernel's roundings; `mut` names one mutation, `drop` the streamed 128-token tile left out."""
    F, N, C = X.shape
    Xf = X.float()
    S = Xf @ Xf.transpose(1, 2)
    keep = torch.ones(N)
    if drop is not None:
        keep[drop * 128:(drop + 1) * 128] = 0

    def lse_used(v):
        if mut == "lse_row_16_below":
            v = _halves_swapped(v)
        if mut == "lse_prev_frame":
            v = v.roll(1, 0)
        return v

    def probs(l):
        P = torch.exp(S - lse_used(l)[..., None])
        return P if mut == "att_not_rounded" else rb(P)

    if op in ("STATS", "ATT"):
        m, l = torch.full((F, N), -float("inf")), torch.zeros(F, N)
        for jt in range(N // 128):
            if jt == drop:
                continue
            st = S[:, :, jt * 128:(jt + 1) * 128]
            mx = torch.maximum(m, st.max(-1).values)
            l = (l if mut == "no_rescale" else l * torch.exp(m - mx)) + torch.exp(st - mx[..., None]).sum(-1)
            m = mx
        out_lse = m + torch.log(l)
        if mut == "lse_row_16_below":
            out_lse = _halves_swapped(out_lse)
        got = {"lse": out_lse}
        if op == "ATT":
            got["out"] = rb(torch.exp(S - out_lse[..., None])).bfloat16()
        return got
    if op == "ATT_FROM_LSE":
        return {"out": rb(torch.exp(S - lse_used(lse)[..., None])).bfloat16()}
    if op == "XR":
        P = probs(lse) * keep[None, :, None]                                   # streamed: the rows i of att
        return {"out": (P.transpose(1, 2) @ Xf).bfloat16()}
    Df = dxr.float()
    G = Xf @ Df.transpose(1, 2)
    rd = rowdot.roll(1, 1) if (mut == "rowdot_neighbour" and rowdot is not None and op != "Y") else rowdot
    if op == "Y":
        y = (probs(lse) * keep[None, None, :]) @ Df
        dot = (Xf * y).sum(-1)
        if mut == "rowdot_neighbour":
            dot = dot.roll(1, 1)
        return {"out": (y if mut == "overwrite" else out0.float() + y).bfloat16(), "rowdot": dot}
    if op in ("DXQ", "DXK"):
        key = (op == "DXK") != (mut == "dxq_dxk_exchanged")
        dS = rb(probs(lse) * (G - rd[..., None]))
        acc = (dS * keep[None, :, None]).transpose(1, 2) @ Xf if key else (dS * keep[None, None, :]) @ Xf
        return {"out": (acc if mut == "overwrite" else out0.float() + acc).bfloat16()}
    if op == "ATT_BWD":
        return {"out": (att_in.float() * (G - rd[..., None])).bfloat16()}
    raise ValueError(op)


_CASES = {}


def _case(family, frames, N, C):
    k = (family, frames, N, C)
    if k not in _CASES:
        _CASES.clear()                                                         # (one at a time: the parametrisation walks them in order)
        _CASES[k] = R.Operands(*k)
    return _CASES[k]


def _check(c, op, got):
    kw = c.operands(op)
    return R.check_op(op, got, c.ref, name="emulation", **kw)


def _survives(c, op, **mut):
    """True when the mutated emulation PASSES the check (which the tests below do not accept)"""
    try:
        _check(c, op, _run(c, op, **mut))
    except AssertionError:
        return False
    return True


def _run(c, op, **mut):
    kw = c.operands(op)
    return emulate(op, c.X, c.dxr, **kw, **mut)


@pytest.mark.parametrize("C", R.CS)
@pytest.mark.parametrize("frames,N", R.SHAPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_honest_emulation_is_inside_every_bound(family, frames, N, C):
    c = _case(family, frames, N, C)
    for op in R.OPS:
        ratio = _check(c, op, _run(c, op))
        RATIOS.setdefault(op, {})[(family, frames, N, C)] = ratio
        print(f"HONEST {op} {frames}x{N}x{C} {family} worst_err_over_bound {ratio:.4f}")
        assert ratio <= 1.0


# mutation -> (ops that have the operand, families in which it must show)
LSE_READERS = ("ATT_FROM_LSE", "XR", "Y", "DXQ", "DXK")
MUTATIONS = {
    "lse_row_16_below": (("STATS", "ATT") + LSE_READERS, ("flat", "peaked", "late_max")),
    "rowdot_neighbour": (("Y", "DXQ", "DXK", "ATT_BWD"), ("flat", "late_max")),
    "lse_prev_frame": (LSE_READERS, ("flat", "frame_scales")),
    "dxq_dxk_exchanged": (("DXQ", "DXK"), ("flat", "late_max")),
    # (early_max: every row's maximum is in the first tile, nothing is ever rescaled, so this mutation is invisible there by construction)
    "no_rescale": (("STATS", "ATT"), ("flat", "late_max")),
    "overwrite": (("Y", "DXQ", "DXK"), ("flat", "late_max")),
}


@pytest.mark.parametrize("C", R.CS)
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_is_rejected(mut, C):
    ops, families = MUTATIONS[mut]
    for family in families:
        c = _case(family, 2, 384, C)
        passed = [op for op in ops if _survives(c, op, mut=mut)]
        assert not passed, f"{mut} passed the check of {passed} at C = {C} in the {family} family: the family cannot show it"


@pytest.mark.parametrize("C", R.CS)
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_a_dropped_streamed_tile_is_rejected(tile, C):
    """first, middle, last of the three tiles of N = 384, in every op that contracts over streamed tiles"""
    for family in ("flat", "late_max"):
        c = _case(family, 2, 384, C)
        passed = [op for op in ("STATS", "ATT", "XR", "Y", "DXQ", "DXK") if _survives(c, op, drop=tile)]
        assert not passed, f"tile {tile} dropped passed the check of {passed} at C = {C} in the {family} family"


@pytest.mark.parametrize("C", R.CS)
def test_att_not_rounded_to_bf16_is_not_a_failure(C):
    """The bf16 rounding of att before the second product is an allowance of the bound, not a demand: a kernel that kept att in fp32
    there is closer to the fp64 reference and passes."""
    for family in ("flat", "late_max"):
        c = _case(family, 2, 384, C)
        for op in ("XR", "Y", "DXQ", "DXK"):
            assert _check(c, op, _run(c, op, mut="att_not_rounded")) <= 1.0


def test_print_worst_honest_ratio_per_op():
    """(runs after the parametrised test above) the table recorded next to the GPU margins in profiles/r19_nxn_strip_margins.txt"""
    assert set(RATIOS) == set(R.OPS), "the honest emulation did not run"
    for op in R.OPS:
        k, v = max(RATIOS[op].items(), key=lambda kv: kv[1])
        print(f"HONEST_WORST {op} {v:.4f} at {k[1]}x{k[2]}x{k[3]} {k[0]}")
