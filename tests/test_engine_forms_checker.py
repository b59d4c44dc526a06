"""What the element-wise fp64 check of the tiled engine's forms (tests/engine_forms_ref.py, used on the GPU by
tests/test_engine_forms_fp64_gpu.py) lets through and what it catches, shown on the CPU at the GPU test's own shapes and inputs.

(a) The kernel's arithmetic emulated in numpy: bf16 products exact in fp32; fp32 operands split into two / three bf16 planes exactly as
    gemm.hip does (round to nearest even, the residual formed in fp32), the three / six plane products the kernel keeps; fp32 x fp32
    products rounded to fp32 on the exact pipe; fp32 accumulation with one rounding per plane product, in two different orders (k by k, and
    32-k blocks summed first and walked backwards).  The epilogues in fp32 as the kernel writes them.  Every case must stay inside its
    bound -- so on the device only the kernel can break it.
(b) Each fault a form could plausibly suffer is REJECTED: a segment dropped, segment 2's B from frame 0 for every frame, segment 3's A
    per group instead of shared, segments 3 and 4 exchanged, b3 and b2 exchanged in the C offset, a slab missing from a kept-slab sum, the
    lse of the neighbouring row, a column tile's part left out of lse, the rescale exp(max_t - max) omitted, MULSUB subtracting lse
    instead of rowdot, D shifted by one row, one element of an fp32 output one bf16 ulp off."""
import numpy as np
import pytest
import torch

from tests import engine_forms_ref as R

F32 = np.float32


# ---- the kernel's arithmetic ---------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32: what (__bf16)x does"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def planes(x, n):
    """gemm.hip: h = (__bf16)x; r = x - (float)h; ... (n planes)"""
    out, r = [], np.asarray(x, dtype=F32)
    for _ in range(n):
        p = bf16_rne(r)
        out.append(p)
        r = (r - p).astype(F32)
    return out


def plane_pairs(A, B, kind):
    """the (A plane, B plane) products the kernel issues, in its order"""
    if kind in ("bf16", "f32"):
        return [(A, B)]
    if kind == "f32s2":
        (ah, al), (bh, bl) = planes(A, 2), planes(B, 2)
        return [(al, bh), (ah, bl), (ah, bh)]
    a, b = planes(A, 3), planes(B, 3)
    return [(a[2], b[0]), (a[1], b[1]), (a[0], b[2]), (a[1], b[0]), (a[0], b[1]), (a[0], b[0])]


def accumulate(acc, A, B, kind, order, k0=0, k1=None):
    """acc += A[..., k0:k1] @ B[..., k0:k1, :] in fp32, one rounding per plane product (order 0) / per 32-k block of one (order 1)"""
    A, B = np.asarray(A, dtype=F32), np.asarray(B, dtype=F32)
    k1 = A.shape[-1] if k1 is None else min(k1, A.shape[-1])
    pairs = plane_pairs(A, B, kind)
    if order == 0:
        for k in range(k0, k1):
            for pa, pb in pairs:
                acc = (acc + (pa[..., :, k:k + 1] * pb[..., k:k + 1, :]).astype(F32)).astype(F32)
    else:
        for kb in reversed(range(k0, k1, 32)):
            ke = min(kb + 32, k1)
            for pa, pb in pairs:
                acc = (acc + np.matmul(pa[..., :, kb:ke], pb[..., kb:ke, :]).astype(F32)).astype(F32)
    return acc


def np_(t):
    return t.float().numpy()


def store(x, bf16):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    return t.bfloat16() if bf16 else t


def seg_emulate(c, order, fault=None):
    A, B = [np_(a) for a in c.A], [np_(b) for b in c.B]
    if fault == "seg2_B_frame0":
        B[1] = np.broadcast_to(B[1][:1], B[1].shape)
    if fault == "seg3_A_per_group":                  # group g reads a block of its own behind the shared one: the next frame's
        A[2] = np.stack([A[2][:, 0], np.roll(A[2][:, 0], -1, axis=0)], 1)
    acc = np.zeros((c.nb1, c.nb2, c.M, c.N), F32)
    for i in range(c.nseg):
        if fault == f"drop_seg{i + 1}":
            continue
        if fault == "seg34_exchanged" and i >= 2:    # A3 against B4 and A4 against B3, over the K they share
            k = min(R.SEG_K[2], R.SEG_K[3])
            acc = accumulate(acc, A[i][..., :k], B[5 - i][..., :k, :], c.kind, order)
            continue
        acc = accumulate(acc, A[i], B[i], c.kind, order)
    v = (acc * F32(c.alpha)).astype(F32)
    if c.with_d:
        D = np_(c.D)
        if fault == "D_row_shift":
            D = np.roll(D, 1, axis=-2)
        v = (v + (np_(c.rs)[..., None] * D).astype(F32)).astype(F32)
    if c.acc:
        v = (v + np_(c.C0)).astype(F32)
    if fault == "bf16_ulp":
        v = v.copy()
        v[1, 1, 37, 41] *= F32(1 + 2.0 ** -7)
    return store(v, c.out_bf16)


# ---- (a) + (b): K segments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_segment_cases_honest_emulation_inside_and_faults_outside(kind):
    worst = 0.0
    for tile, c in R.seg_cases(only_kind=kind):
        ref, bound = c.ref()
        for order in (0, 1):
            worst = max(worst, R.check_bound(seg_emulate(c, order), ref, bound, f"{c.name} order {order}"))
        if tile not in (0, 128):                     # the faults once per (form, small shape, big shape); every output type and term comes by
            continue
        faults = [f"drop_seg{i + 1}" for i in range(c.nseg)] + ["seg2_B_frame0"]
        if c.nseg >= 3:
            faults.append("seg3_A_per_group")
        if c.nseg == 4:
            faults.append("seg34_exchanged")
        if c.with_d:
            faults.append("D_row_shift")
        if not c.out_bf16:
            faults.append("bf16_ulp")
        for f in faults:
            with pytest.raises(R.ProductMismatch):
                R.check_bound(seg_emulate(c, 0, f), ref, bound, f"{c.name} {f}")
    print(f"MARGIN emulated segments {kind} worst_err_over_bound {worst:.4f}")
    assert worst <= 1.0


def test_every_segment_fault_was_tried():
    """the walk of seg_cases over output type / D / accumulate gives every fault of the list a case at tile 0 or 128"""
    cs = [c for t, c in R.seg_cases() if t in (0, 128)]
    assert any(c.nseg == 4 for c in cs) and any(c.nseg >= 3 for c in cs)
    assert any(c.with_d for c in cs) and any(not c.out_bf16 for c in cs) and any(c.out_bf16 for c in cs)


# ---- third batch level, kept slabs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(R.KINDS))
@pytest.mark.parametrize("out_bf16", [False, True])
def test_third_batch_level(kind, out_bf16):
    c = R.Nb3Case(kind, out_bf16)
    ref, bound = c.ref()
    for order in (0, 1):
        acc = accumulate(np.zeros(ref.shape, F32), np_(c.A), np_(c.B), kind, order)
        assert R.check_bound(store(acc, out_bf16), ref, bound, c.name) <= 1.0
    # split-K: three slabs of 64 / 128 (bf16) K entries, then the reduce
    per = 128 if kind == "bf16" else 64
    slabs = [accumulate(np.zeros(ref.shape, F32), np_(c.A), np_(c.B), kind, 0, k, k + per) for k in range(0, 3 * per, per)]
    red = ((slabs[0] + slabs[1]).astype(F32) + slabs[2]).astype(F32)
    assert R.check_bound(store(red, out_bf16), ref, bound, c.name + " ksplit 3") <= 1.0
    with pytest.raises(R.ProductMismatch):           # b3 and b2 exchanged in the C offset (nb3 == nb2 == 2: the blocks change places)
        R.check_bound(store(acc, out_bf16).transpose(1, 2), ref, bound, c.name + " b3 <-> b2")


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_kept_slabs(kind):
    c = R.SlabCase(kind)
    ref, bound = c.ref()
    per = c.kper()
    slabs = [accumulate(np.zeros(ref.shape, F32), np_(c.A), np_(c.B), kind, 1, s * per, (s + 1) * per) if s * per < c.K else np.zeros(ref.shape, F32)
             for s in range(c.ksplit)]
    total = torch.from_numpy(np.stack(slabs)).double().sum(0)
    assert R.check_bound(total, ref, bound, c.name) <= 1.0
    with pytest.raises(R.ProductMismatch):           # one slab missing from the sum
        R.check_bound(total - torch.from_numpy(slabs[2]).double(), ref, bound, c.name + " without slab 2")


# ---- softmax epilogues -----------------------------------------------------------------------------------------------------------------------
def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32))


def rowstats_emulate(v, tiles):
    """(F, M, tiles, 2): per tile the max, and the sum of exp(v - max) as two threads' 64-column sums added"""
    out = []
    for t in range(tiles):
        sl = v[..., t * R.TILE:(t + 1) * R.TILE]
        mx = sl.max(-1).values
        e = torch.exp(sl - mx[..., None])
        out.append(torch.stack([mx, e[..., :64].sum(-1) + e[..., 64:].sum(-1)], -1))
    return torch.stack(out, -2)


def row_lse_emulate(parts, fault=None):
    mx_t, sm_t = parts[..., 0], parts[..., 1]
    if fault == "tile_left_out":
        mx_t, sm_t = mx_t[..., :-1], sm_t[..., :-1]
    mx = mx_t.max(-1, keepdim=True).values
    w = sm_t if fault == "no_rescale" else sm_t * torch.exp(mx_t - mx)
    lse = mx[..., 0] + torch.log(w.sum(-1))
    return lse.roll(1, -1) if fault == "neighbour_row" else lse


@pytest.mark.parametrize("kind", R.SOFTMAX_KINDS)
@pytest.mark.parametrize("family,shape", R.softmax_ids())
def test_softmax_epilogues(kind, family, shape):
    c = R.SoftmaxCase(kind, family, shape)
    A, Bt = np_(c.A), np.ascontiguousarray(np_(c.B).transpose(0, 2, 1))
    out_bf16 = kind == "bf16"
    for order in (0, 1):
        acc = t32(accumulate(np.zeros((shape[0], shape[1], shape[2]), F32), A, Bt, kind, order))
        for alpha in (1.0, 0.5):
            r = c.at(alpha)
            v = acc * alpha
            name = f"{c.name} alpha {alpha} order {order}"
            parts = rowstats_emulate(v, c.tiles)
            (mr, mb), (sr, sb) = r.parts(parts[..., 0])
            assert R.check_bound(parts[..., 0], mr, mb, name + " max") <= 1.0
            assert R.check_bound(parts[..., 1], sr, sb, name + " sum") <= 1.0
            lse = row_lse_emulate(parts)
            lref, lbound = R.row_lse_ref(parts)
            assert R.check_bound(lse, lref, lbound, name + " lse of its parts") <= 1.0
            assert R.check_bound(lse, r.lse_true, R.lse_from_scores_bound(parts, sr, sb), name + " lse of the scores") <= 1.0
            ex = torch.exp(v - r.lse_in[..., None])
            assert R.check_bound(ex.bfloat16() if out_bf16 else ex, *r.exp(r.lse_in), name + " EXP") <= 1.0
            ms = c.D.float() * (v - r.rowdot[..., None])
            assert R.check_bound(ms.bfloat16() if out_bf16 else ms, *r.mulsub(r.rowdot, c.D), name + " MULSUB") <= 1.0
            if order:
                continue
            # ---- faults --------------------------------------------------------------------------------------------------------------
            faults = ["neighbour_row"] + (["tile_left_out", "no_rescale"] if c.tiles > 1 else [])
            for f in faults:
                bad = row_lse_emulate(parts, f)
                with pytest.raises(R.ProductMismatch):
                    R.check_bound(bad, lref, lbound, name + f" {f} (parts)")
                with pytest.raises(R.ProductMismatch):
                    R.check_bound(bad, r.lse_true, R.lse_from_scores_bound(parts, sr, sb), name + f" {f} (scores)")
            bad = torch.exp(v - r.lse_in.roll(1, -1)[..., None])         # EXP with the neighbouring row's lse
            with pytest.raises(R.ProductMismatch):
                R.check_bound(bad.bfloat16() if out_bf16 else bad, *r.exp(r.lse_in), name + " EXP neighbour row")
            bad = c.D.float() * (v - r.lse_in[..., None])                # MULSUB subtracting lse instead of rowdot
            with pytest.raises(R.ProductMismatch):
                R.check_bound(bad.bfloat16() if out_bf16 else bad, *r.mulsub(r.rowdot, c.D), name + " MULSUB - lse")
            bad = c.D.float().roll(1, -2) * (v - r.rowdot[..., None])    # D shifted by one row
            with pytest.raises(R.ProductMismatch):
                R.check_bound(bad.bfloat16() if out_bf16 else bad, *r.mulsub(r.rowdot, c.D), name + " MULSUB D row shift")
            if not out_bf16:                                             # right, but one bf16 ulp off in an fp32 output
                bad = ex.clone()
                bad[0, 3, 5] *= 1 + 2.0 ** -7
                with pytest.raises(R.ProductMismatch, match="1 of"):
                    R.check_bound(bad, *r.exp(r.lse_in), name + " EXP one bf16 ulp")


@pytest.mark.parametrize("what,rows,tiles", R.LSE_ALONE)
def test_row_lse_on_constructed_parts(what, rows, tiles):
    parts = R.lse_alone_parts(what, rows, tiles)
    ref, bound = R.row_lse_ref(parts)
    assert R.check_bound(row_lse_emulate(parts), ref, bound, what) <= 1.0
    if tiles > 1 and "150" not in what:
        for f in ("tile_left_out", "no_rescale"):
            with pytest.raises(R.ProductMismatch):
                R.check_bound(row_lse_emulate(parts, f), ref, bound, f"{what} {f}")
    if "150" in what:                                # the underflowing tile must not matter: dropping IT is inside the bound ...
        keep = torch.cat([parts[:, :1], parts[:, 2:]], 1)
        assert R.check_bound(row_lse_emulate(keep), ref, bound, what + " without the underflowing tile") <= 1.0
        with pytest.raises(R.ProductMismatch):       # ... but adding it unscaled is not
            R.check_bound(row_lse_emulate(parts, "no_rescale"), ref, bound, what + " no_rescale")


def test_three_plane_term_is_derived_not_quoted():
    """The derived worst case of the three-plane split holds on 200 000 random pairs, the third plane leaves nothing of x, and single
    products exceed the figure quoted in csrc/gemm.h several times over: a bound set from that figure would reject a correct kernel."""
    g = torch.Generator().manual_seed(1)
    x = (1.0 + torch.rand(200000, generator=g)).numpy().astype(F32)
    y = (1.0 + torch.rand(200000, generator=g)).numpy().astype(F32)
    a, b = planes(x, 3), planes(y, 3)
    assert np.array_equal((a[0].astype(np.float64) + a[1]) + a[2], x.astype(np.float64))
    kept = sum(a[i].astype(np.float64) * b[j].astype(np.float64) for i, j in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)))
    rel = np.abs(kept - x.astype(np.float64) * y.astype(np.float64)) / (x.astype(np.float64) * y.astype(np.float64))
    assert rel.max() <= R.EPS_PLANES3
    assert rel.max() > 4 * R.GEMM_H_QUOTED_PLANES3, rel.max()
