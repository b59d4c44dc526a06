"""The strip kernels of the AVVP N x N block (csrc/nxn_att.hip: k_nxn_att, k_nxn_xr, k_nxn_y, k_nxn_dxq / k_nxn_dxk, and k_nxn_att with the
softmax stored / k_nxn_att_bwd, which no site call reaches without a development switch) checked ONE BY ONE, element by element, against
fp64 recomputed from the operands exactly as each kernel read them, through avmoe_nxn_strip (include/avmoe.h).  The bounds are those of
tests/nxn_ref.py, counted from the kernel text; tests/test_nxn_checker.py shows on the CPU what such a check catches (a streamed tile
left out, the log-sum-exp of the row 16 below, the neighbouring row's row dot, another frame's log-sum-exp, the two dS products
exchanged, the running sum not rescaled, `out` overwritten).

Why one by one: inside a site neither att nor dS is ever in memory, the three backward kernels read-modify-write dX in bf16 behind the
site's own dX product and k_nxn_axpy, and sections 32 / 64 of avmoe_moe_backward_part refuse N x N sites, so the backward cannot be
stopped between the kernels.  And the inputs the whole-site comparisons draw (0.3 randn) make the softmax nearly the identity: at C = 192
the two dS products sit below one bf16 ulp of dX there.  Here the operands are free inputs, chosen so that rows, tiles and frames tell each
other apart: the `flat` family (0.1 randn: attention near uniform, every key counts), per-row offsets on the log-sum-exp, row dots drawn
per row, frames at different scales, maxima placed in the last / first key tile (scores up to ~170: most exponentials underflow).

The last test runs the same kernels as a site launches them (MoeRun, profiler on) and checks what the workspace keeps: nlse, xr, sxr after
the forward, nrd after sections 1 and 2 -- also with the frames in chunks.  The site's final dX is deliberately NOT bounded here: it is a
five-term bf16 read-modify-write chain in which the two dS terms sit at or below a bf16 ulp of the total, which is exactly why the entry
point above exists."""
import ctypes as C_

import pytest
import torch

from tests import nxn_ref as R
from tests.stream_product_ref import check_bound, check_untouched

pytestmark = pytest.mark.gpu

CHECKED = {}       # op -> {(C, frames, N, family): worst err / bound}
PAD = 256          # guard band, elements
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2       # include/avmoe.h


def _dev():
    return torch.device("cuda:0")


class Guarded:
    """A device buffer between two guard bands holding a sentinel (all bits set: NaN in fp32 and bf16)"""

    def __init__(self, shape, dtype, init=None):
        n = 1
        for k in shape:
            n *= k
        self.ity = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.raw = torch.empty(n + 2 * PAD, dtype=dtype, device=_dev())
        self.raw.view(self.ity).fill_(-1)
        self.n, self.t = n, self.raw[PAD:PAD + n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def bits(self):
        return self.t.contiguous().view(self.ity).clone()

    def intact(self, name):
        r = self.raw.view(self.ity)
        check_untouched(torch.cat([r[:PAD], r[PAD + self.n:]]), -1, f"{name}: guard bands")

    def poisoned(self):
        return bool((self.raw.view(self.ity) == -1).all())


def _ptr(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def strip(op, X, dxr, frames, N, C, lse, rowdot, out, att_in):
    from avmoe_amd import _capi, _capi_moe as cm
    L = _capi.lib()
    assert hasattr(L, "avmoe_nxn_strip"), "the library does not export avmoe_nxn_strip"
    st = L.avmoe_nxn_strip(cm.NXN_OP[op], _ptr(X), _ptr(dxr), frames, N, C, _ptr(lse), _ptr(rowdot), _ptr(out), _ptr(att_in),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def run_op(op, X, dxr=None, lse=None, rowdot=None, out0=None, att_in=None):
    """One call on fresh guarded outputs -> ({"lse" / "rowdot" / "out": Guarded}, status).  Inputs the op only reads are passed as they are."""
    F, N, C = X.shape
    out = {}
    lse_a, rd_a, out_a = lse, rowdot, None
    if op in ("STATS", "ATT"):
        lse_a = out["lse"] = Guarded((F, N), torch.float32)
    if op == "Y":
        rd_a = out["rowdot"] = Guarded((F, N), torch.float32)
    if op in ("ATT", "ATT_FROM_LSE", "ATT_BWD"):
        out_a = out["out"] = Guarded((F, N, N), torch.bfloat16)
    elif op == "XR":
        out_a = out["out"] = Guarded((F, N, C), torch.bfloat16)
    elif op in ("Y", "DXQ", "DXK"):
        out_a = out["out"] = Guarded((F, N, C), torch.bfloat16, init=out0)
    st = strip(op, X, dxr, F, N, C, lse_a, rd_a, out_a, att_in)
    return out, st


def _values(gd):
    return {k: v.t for k, v in gd.items()}


class Rec:
    """Every op of a case is tried; the test fails at the end with all mismatches"""

    def __init__(self, key):
        self.key, self.fail = key, []          # key = (C, frames, N, family)

    def check(self, op, tag, fn):
        C, F, N, fam = self.key
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{op} [{tag}]: {e}")
            return
        prev = CHECKED.setdefault(op, {}).get(self.key, 0.0)
        CHECKED[op][self.key] = max(prev, ratio)
        print(f"MARGIN {op} {F}x{N}x{C} {fam} {tag} worst_err_over_bound {ratio:.4f}")

    def finish(self):
        assert not self.fail, "\n".join(self.fail)


def _checked_call(rec, c, op, tag, **kw):
    """run the op twice on the same operands: status, bound, guard bands, finite (check_bound), second call bit-identical"""
    gd, st = run_op(op, c.X, c.dxr, **kw)
    assert st == OK, (op, st)
    name = f"{rec.key} {tag}"
    rec.check(op, tag, lambda: R.check_op(op, _values(gd), c.ref, name=name, **kw))
    gd2, st2 = run_op(op, c.X, c.dxr, **kw)
    assert st2 == OK
    for k, v in gd.items():
        try:
            v.intact(f"{op} {k}")
            assert torch.equal(v.bits(), gd2[k].bits()), f"{op} {k}: a second call on the same operands gives other bits"
        except AssertionError as e:
            rec.fail.append(f"{op} [{tag}]: {e}")
    return gd


@pytest.mark.parametrize("C", R.CS)
@pytest.mark.parametrize("frames,N", R.SHAPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_every_op_against_fp64(family, frames, N, C):
    c = R.Operands(family, frames, N, C, device=_dev())
    rec = Rec((C, frames, N, family))
    zeros = torch.zeros_like(c.X)
    # ---- the forward's statistics; the softmax stored (development path) -----------------------------------------------------------------
    stats = _checked_call(rec, c, "STATS", "own")
    att = _checked_call(rec, c, "ATT", "own")
    assert torch.equal(stats["lse"].bits(), att["lse"].bits()), "STATS and ATT write different lse"
    lse_k = stats["lse"].t.clone()
    again, st = run_op("ATT_FROM_LSE", c.X, lse=lse_k)
    assert st == OK and torch.equal(again["out"].bits(), att["out"].bits()), "ATT_FROM_LSE on ATT's lse does not give ATT's att bit for bit"
    # ---- every reader of lse on lse = fl32(fp64 lse) + a per-row offset; every reader of rowdot on row dots drawn per row -------------------
    _checked_call(rec, c, "ATT_FROM_LSE", "lse+delta", **c.operands("ATT_FROM_LSE"))
    _checked_call(rec, c, "XR", "lse+delta", **c.operands("XR"))
    for tag, out0 in (("zero_out", zeros), ("prefilled_out", c.out0)):
        for op in ("Y", "DXQ", "DXK"):
            kw = c.operands(op)
            kw["out0"] = out0
            _checked_call(rec, c, op, f"lse+delta {tag}", **kw)
    _checked_call(rec, c, "ATT_BWD", "drawn rowdot", **c.operands("ATT_BWD"))
    # ---- Y -> DXQ -> DXK as the backward chains them, on the kernel's own lse and rowdot: each step from the operands the one before left ----
    gy = _checked_call(rec, c, "Y", "chain", lse=lse_k, out0=c.out0)
    rd_k, out1 = gy["rowdot"].t.clone(), gy["out"].t.clone()
    gq = _checked_call(rec, c, "DXQ", "chain", lse=lse_k, rowdot=rd_k, out0=out1)
    _checked_call(rec, c, "DXK", "chain", lse=lse_k, rowdot=rd_k, out0=gq["out"].t.clone())
    rec.finish()


@pytest.mark.parametrize("C", R.CS)
def test_three_frames_are_three_calls_of_one_frame(C):
    """frames = 3 gives, frame by frame, the bits of three calls with frames = 1: every op (frames at different scales)"""
    c = R.Operands("frame_scales", 3, 256, C, device=_dev())
    for op in R.OPS:
        kw = c.operands(op)
        whole, st = run_op(op, c.X, c.dxr, **kw)
        assert st == OK
        for f in range(3):
            one, st = run_op(op, c.X[f:f + 1].contiguous(), c.dxr[f:f + 1].contiguous(), **{k: v[f:f + 1].contiguous() for k, v in kw.items()})
            assert st == OK
            for k, v in one.items():
                assert torch.equal(v.bits()[0], whole[k].bits()[f]), f"{op} {k}: frame {f} of a three-frame call differs from its own call"
                v.intact(f"{op} {k}")


@pytest.mark.parametrize("C", R.CS)
def test_zero_gradient_leaves_out_bit_for_bit(C):
    """dxr == 0 with rowdot == 0: Y, DXQ, DXK leave a prefilled out as it is, and Y writes rowdot = +0 / -0"""
    c = R.Operands("flat", 2, 384, C, device=_dev())
    zd, zr = torch.zeros_like(c.dxr), torch.zeros_like(c.rowdot)
    for op in ("Y", "DXQ", "DXK"):
        g0 = Guarded(c.out0.shape, torch.bfloat16, init=c.out0)
        gd, st = run_op(op, c.X, zd, lse=c.lse, rowdot=None if op == "Y" else zr, out0=c.out0)
        assert st == OK
        assert torch.equal(gd["out"].bits(), g0.bits()), f"{op}: out changed under a zero gradient"
        if op == "Y":
            assert bool((gd["rowdot"].t == 0).all()), "Y: rowdot != 0 under a zero gradient"
        for k, v in gd.items():
            v.intact(f"{op} {k}")


def _needs(op):
    """the pointers an op uses (include/avmoe.h)"""
    return {"STATS": ("X", "lse"), "ATT": ("X", "lse", "out"), "ATT_FROM_LSE": ("X", "lse", "out"), "XR": ("X", "lse", "out"),
            "Y": ("X", "dxr", "lse", "rowdot", "out"), "DXQ": ("X", "dxr", "lse", "rowdot", "out"), "DXK": ("X", "dxr", "lse", "rowdot", "out"),
            "ATT_BWD": ("X", "dxr", "rowdot", "out", "att_in")}[op]


def test_refusals_launch_nothing():
    """C = 128, N = 200, N = 0 (AVMOE_ERR_UNSUPPORTED, from the wrappers' own check) and a NULL operand (AVMOE_ERR_BAD_ARG): the documented
    status, no kernel launched (profiler) and poisoned outputs stay poisoned"""
    from avmoe_amd import _capi
    L = _capi.lib()
    dev = _dev()
    X = (0.1 * torch.randn(1, 256, 192, device=dev)).bfloat16()
    dxr = X.clone()
    att_in = torch.zeros(1, 256, 256, device=dev, dtype=torch.bfloat16)
    L.avmoe_prof_reset(); L.avmoe_prof_enable(1)
    try:
        for op in R.OPS:
            cases = [("C = 128", dict(N=128, C=128), UNSUPPORTED, None), ("N = 200", dict(N=200, C=96), UNSUPPORTED, None),
                     ("N = 0", dict(N=0, C=96), UNSUPPORTED, None)] + [(f"{p} NULL", dict(N=256, C=192), BAD_ARG, p) for p in _needs(op)]
            for what, shp, want, null in cases:
                bufs = {"X": X, "dxr": dxr, "att_in": att_in, "lse": Guarded((1, 256), torch.float32), "rowdot": Guarded((1, 256), torch.float32),
                        "out": Guarded((1, 256, 256), torch.bfloat16)}
                a = dict(bufs)
                if null:
                    a[null] = None
                st = strip(op, a["X"], a["dxr"], 1, shp["N"], shp["C"], a["lse"], a["rowdot"], a["out"], a["att_in"])
                assert st == want, f"{op} with {what}: status {st}, documented {want} ({L.avmoe_last_error().decode()})"
                assert all(bufs[k].poisoned() for k in ("lse", "rowdot", "out")), f"{op} with {what}: an output was written"
        assert strip("STATS", X, None, 1, 256, 192, Guarded((1, 256), torch.float32), None, None, None) == OK      # (unused pointers may be NULL)
        L.avmoe_prof_reset()
        assert L.avmoe_nxn_strip(99, X.data_ptr(), None, 1, 256, 192, None, None, None, None, None) == BAD_ARG
        for op in R.OPS:                                           # frames = 0: AVMOE_OK without a launch
            o = Guarded((1, 256, 256), torch.bfloat16)
            l, r = Guarded((1, 256), torch.float32), Guarded((1, 256), torch.float32)
            assert strip(op, X, dxr, 0, 256, 192, l, r, o, att_in) == OK and o.poisoned() and l.poisoned() and r.poisoned(), op
        torch.cuda.synchronize()
        ran = {f["name"] for f in _capi.prof_report()}
        assert not ran, f"a refused call launched {ran}"
    finally:
        L.avmoe_prof_enable(0); L.avmoe_prof_reset()


def test_every_strip_op_was_checked():
    """Closes the module: each of the eight ops was checked against fp64 at both C, at N = 384, in the `flat` and the `late_max` family.
    (Runs after the tests above: it fails when they did not run.)"""
    missing = []
    for op in R.OPS:
        got = CHECKED.get(op, {})
        for C in R.CS:
            for fam in ("flat", "late_max"):
                if (C, 2, 384, fam) not in got:
                    missing.append((op, C, fam))
        for (C, F, N, fam), ratio in sorted(got.items()):
            print(f"COVERED {op} {F}x{N}x{C} {fam} {ratio:.4f}")
        if got:
            k, v = max(got.items(), key=lambda kv: kv[1])
            print(f"MARGIN_WORST {op} {v:.4f} at {k[1]}x{k[2]}x{k[0]} {k[3]}")
    assert not missing, f"ops not checked at N = 384 in both families and both C: {missing}"


# ---- the same kernels as a site launches them -----------------------------------------------------------------------------------------------
class NxnSite:
    """One bf16 training-mode AVVP site (tests/moe_gpu_util.py::MoeRun: NaN-poisoned workspaces, guard bands), the backward in sections"""

    def __init__(self, C, S=3, N=256, seed=11):
        from oracle import avmoe_oracle as O
        from tests.moe_gpu_util import MoeRun
        cfg = O.AdapterConfig(Cx=C, Nx=N, Cy=288 - C, Ny=128, reduction=8, groups=2, K=32, variant="avvp", lb_loss=True)
        P, B = O.init_params(cfg, seed=seed)
        g = torch.Generator().manual_seed(seed + 100)
        X = 0.1 * torch.randn(S, N, C, generator=g)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
        self.G = torch.randn(S, N, C, generator=g)
        self.cfg, self.S, self.N, self.C = cfg, S, N, C
        self.run = MoeRun(cfg, P, B, X, Y, bf16=True, training=True)

    def dev(self, name, dtype, shape):
        region, off, nbytes = self.run.table[name]
        raw = (self.run.saved if region == 0 else self.run.scratch)[off:off + nbytes]
        n = 1
        for k in shape:
            n *= k
        return raw.view(dtype)[:n].reshape(shape)

    def begin_backward(self):
        from avmoe_amd import _capi_moe as cm
        r = self.run
        r.dOut = self.G.to(r.dev, r.tdt).contiguous()
        r.dX = torch.full_like(r.X, float("nan"))
        r.dY = torch.full_like(r.Y, float("nan"))
        r.grads = {k: torch.full_like(v, float("nan")) for k, v in r.params.items()}
        r.gptrs = cm.make_ptrs(r.grads, self.cfg.E_m, self.cfg.E_s)
        r.lbw = torch.zeros(1, device=r.dev, dtype=torch.float32)

    def part(self, parts):
        from avmoe_amd import _capi as capi
        r = self.run
        st = r.L.avmoe_moe_backward_part(C_.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C_.byref(r.ptrs), r.dOut.data_ptr(), r.lbw.data_ptr(),
                                         r.saved.data_ptr(), r.scratch.data_ptr(), r.dX.data_ptr(), r.dY.data_ptr(), C_.byref(r.gptrs), int(parts),
                                         torch.cuda.current_stream().cuda_stream)
        capi.check(st, f"avmoe_moe_backward_part({parts})")
        torch.cuda.synchronize()


def _names(capi, L):
    torch.cuda.synchronize()
    ran = {f["name"] for f in capi.prof_report()}
    L.avmoe_prof_reset()
    return ran


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("C", R.CS)
def test_strip_kernels_as_a_site_launches_them(C, chunk, avmoe_hooks):
    """nlse, xr, sxr after the forward and nrd after sections 1 and 2 of the backward, from the workspace of one AVVP site (3 frames of 256
    tokens, X = 0.1 randn), each against fp64 from the operands as stored; chunk = 2: the frames in chunks of 2 + 1, where nrd holds the
    last chunk's rows only."""
    from avmoe_amd import _capi
    L = _capi.lib()
    if chunk:
        avmoe_hooks(0, chunk)
    L.avmoe_prof_reset(); L.avmoe_prof_enable(1)
    try:
        s = NxnSite(C)
        S, N = s.S, s.N
        s.run.forward()
        ran = _names(_capi, L)
        assert "k_nxn_att" in ran and "k_nxn_xr" in ran, ran
        X = s.run.X
        ref = R.NxnRef(X)
        nlse = s.dev("nlse", torch.float32, (S, N))
        xr = s.dev("xr", torch.bfloat16, (S, N, C))
        tag = f"site C = {C} chunk = {chunk}"
        w = [check_bound(nlse, *ref.lse(), f"{tag} nlse (frame, row)"),
             check_bound(xr, *ref.xr(nlse), f"{tag} xr (frame, row, channel)"),
             check_bound(s.dev("sxr", torch.float32, (3, S * N)), *R.xrstats_ref(X.reshape(S * N, C), xr.reshape(S * N, C)), f"{tag} sxr ([sum, sum of squares, x . xr], token)")]
        s.begin_backward()
        s.part(1)
        s.part(2)
        ran |= _names(_capi, L)
        assert all(k in ran for k in ("k_nxn_y", "k_nxn_dxq", "k_nxn_dxk")), ran
        assert "k_nxn_att_bwd" not in ran and "k_nxn_rowdot" not in ran, ran
        dxr = s.dev("dxr", torch.bfloat16, (S, N, C))
        f0 = 2 if chunk else 0                                     # chunks of 2 + 1 frames: the last chunk is frame 2 alone
        sub = R.NxnRef(X[f0:], dxr[f0:])
        lse_sub = nlse[f0:].contiguous()
        rd, erd = sub.y(lse_sub, torch.zeros_like(X[f0:]))["rowdot"]
        w.append(check_bound(s.dev("nrd", torch.float32, (S - f0, N)), rd, erd, f"{tag} nrd (frame of the last chunk, row)"))
        print(f"MARGIN site C={C} chunk={chunk} nlse {w[0]:.4f} xr {w[1]:.4f} sxr {w[2]:.4f} nrd {w[3]:.4f}")
        assert s.run.guards_intact(), "a kernel wrote past its workspace"
        assert torch.isfinite(s.run.out.float()).all() and torch.isfinite(s.run.dX.float()).all()
    finally:
        L.avmoe_prof_enable(0); L.avmoe_prof_reset()
