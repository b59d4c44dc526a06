"""The forms of the tiled engine (csrc/gemm.hip, launch_gemm) that avmoe_gemm_desc has no field for -- further K segments, the third batch
level, kept split-K slabs, the softmax epilogues and gemm_row_lse -- each run ALONE through avmoe_gemm_form / avmoe_gemm_row_lse
(include/avmoe.h, tests only) on operands of the test's choosing, and every output element checked against fp64 of exactly those operands
(they go to the device as stored; the fp64 products stay there).  References, bounds and the cases: tests/engine_forms_ref.py;
tests/test_engine_forms_checker.py shows on the CPU that an honest emulation of the kernel passes at these inputs and which faults fail.

Inside a site these forms are guarded only by the whole-site comparison with the oracle, which is blind for the N x N block
(DESIGN_CURRENT.md section 2) and compares the multi-segment dX product at max-norm tolerances.

Every operand sits in a buffer of its own between guard bands, with leading dimensions and batch strides of its own; what the kernel may
not read (behind the last k-row of an MN-major operand, beyond the readable K padding of a K-major one, the gaps between the batches) and
what it may not write (C outside the (M, N) blocks) holds a sentinel -- all bits set, NaN in fp32 and bf16 -- that must neither leak nor be
overwritten.  The readable K padding of a K-major operand is finite, zero on one side (csrc/gemm.h).  Every test reads the profiler report
and asserts WHICH kernel ran: the tiled engine's instance, not gemm_stream / gemm_frames.  Every call is made twice: same bytes."""
import ctypes as C_

import pytest
import torch

from tests import engine_forms_ref as R

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2       # include/avmoe.h
FRONT = 64                                 # guard band, elements (a multiple of 16 bytes in every type)
MARGINS = {}


def _dev():
    return torch.device("cuda:0")


def _ity(dtype):
    return torch.int16 if dtype == torch.bfloat16 else torch.int32


def margin(name, ratio):
    MARGINS[name] = max(MARGINS.get(name, 0.0), ratio)
    print(f"MARGIN {name} worst_err_over_bound {ratio:.4f}")


class Placed:
    """A tensor (*batch, R, Cn) in a flat device buffer of its own: row stride ld, `pad_rows` sentinel rows behind each block, batch strides
    grown from the inside out with a gap (elements) behind each level; everything but the blocks holds the sentinel.  t=None: an output."""

    def __init__(self, shape, dtype, *, ld, pad_rows=2, gaps=None, t=None, strides=None):
        batch, (Rr, Cn) = tuple(shape[:-2]), shape[-2:]
        if strides is None:
            gaps = gaps or [8 * (i + 1) for i in range(len(batch))]
            strides, s = [], (Rr + pad_rows) * ld
            for n, gp in zip(reversed(batch), gaps):
                s += gp
                strides.append(s)
                s *= n
            strides = tuple(reversed(strides))
            total = s
        else:
            total = sum(st * (n - 1) for st, n in zip(strides, batch)) + Rr * ld
        self.shape, self.ld, self.strides, self.dtype = tuple(shape), ld, tuple(strides), dtype
        self.flat = torch.empty(2 * FRONT + total, dtype=dtype, device=_dev())
        self.flat.view(_ity(dtype)).fill_(-1)
        if t is not None:
            self.view().copy_(t)

    def view(self, flat=None, cols=None, col0=0):
        f = self.flat if flat is None else flat
        shape = self.shape if cols is None else self.shape[:-1] + (cols,)
        return f.as_strided(shape, self.strides + (self.ld, 1), FRONT + col0)

    def fill_cols(self, col0, cols, value):
        """the readable K padding of a K-major operand"""
        if cols > 0:
            self.view(cols=cols, col0=col0).fill_(value)

    def ptr(self):
        return self.flat.data_ptr() + FRONT * self.flat.element_size()

    def bits(self):
        return self.flat.view(_ity(self.dtype)).clone()

    def untouched_outside(self, name):
        """everything but the blocks still holds the sentinel"""
        b = self.bits()
        self.view(flat=b).fill_(-1)
        R.check_untouched(b, -1, f"{name}: outside the (M, N) blocks")

    def poisoned(self):
        return bool((self.flat.view(_ity(self.dtype)) == -1).all())


def _ru(x, m):
    return -(-x // m) * m


def place_operand(t, mn_major, kind, kpad=0.0):
    """t as stored (stored_A / stored_B): K-major (*batch, rows, K), MN-major (*batch, K, rows).  ld = the contiguous extent rounded up to 8
    plus 8; a K-major operand's readable padding (up to a multiple of 16 bytes) is filled with kpad, everything else keeps the sentinel."""
    epc = 8 if kind == "bf16" else 4
    Rr, Cn = t.shape[-2:]
    p = Placed(t.shape, t.dtype, ld=_ru(Cn, 8) + 8, t=t)
    if not mn_major:
        p.fill_cols(Cn, _ru(Cn, epc) - Cn, kpad)
    return p


def stored_A(a, mn):        # a: (*batch, M, K)
    return a.transpose(-1, -2).contiguous() if mn else a


def stored_B(b, mn):        # b: (*batch, K, N)
    return b if mn else b.transpose(-1, -2).contiguous()


def base_desc(**kw):
    from avmoe_amd import _capi
    d = _capi.GemmFormDesc()
    d.base.nb1 = d.base.nb2 = 1
    d.base.alpha = 1.0
    d.base.sCj = 1
    d.base.ksplit = 1
    d.nb3 = 1
    for k, v in kw.items():
        if k in ("nb3", "epi", "keep_slabs", "sA3", "sB3", "sC3"):
            setattr(d, k, v)
        else:
            setattr(d.base, k, v)
    return d


def set_kind(d, kind, out_bf16):
    d.base.dtype, d.base.fp32_planes = R.KINDS[kind][0], {0: 0, 1: 3, 2: 2}[R.KINDS[kind][1]]
    d.base.out_dtype = 1 if out_bf16 else 0


def _p(x):
    if x is None:
        return None
    return x.ptr() if isinstance(x, Placed) else (x.data_ptr() if hasattr(x, "data_ptr") else x)


def call(d, A, B, Cc, rs=None, D=None, ws=None, row_part=None, row_lse=None):
    from avmoe_amd import _capi
    L = _capi.lib()
    assert hasattr(L, "avmoe_gemm_form"), "the library does not export avmoe_gemm_form"
    arr = lambda v: (C_.c_void_p * 4)(*[_p(x) for x in (list(v) + [None] * 4)[:4]])
    a, b = arr(A), arr(B)
    st = L.avmoe_gemm_form(C_.byref(d), C_.byref(a), C_.byref(b), _p(Cc), _p(rs), _p(D), _p(ws), _p(row_part), _p(row_lse),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def row_lse(parts, rows, tiles, lse):
    from avmoe_amd import _capi
    st = _capi.lib().avmoe_gemm_row_lse(_p(parts), rows, tiles, _p(lse), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


@pytest.fixture
def prof():
    """profiler on for the test; prof() -> the kernel families launched since the last look"""
    from avmoe_amd import _capi
    L = _capi.lib()
    L.avmoe_prof_reset(); L.avmoe_prof_enable(1)

    def ran():
        torch.cuda.synchronize()
        names = {f["name"] for f in _capi.prof_report()}
        L.avmoe_prof_reset()
        return names
    try:
        yield ran
    finally:
        L.avmoe_prof_enable(0); L.avmoe_prof_reset()


def last_error():
    from avmoe_amd import _capi
    m = _capi.lib().avmoe_last_error()
    return m.decode() if m else ""


def twice(fn, outs, name):
    """fn() fills the outputs `outs` (Placed / tensors); a second call on the same operands gives the same bytes"""
    def snap():
        return [o.bits() if isinstance(o, Placed) else o.clone().view(_ity(o.dtype)) for o in outs]
    assert fn() == OK, (name, last_error())
    first = snap()
    assert fn() == OK, (name, last_error())
    for x, y in zip(first, snap()):
        assert torch.equal(x, y), f"{name}: a second call on the same operands gives other bits"


# ---- K segments ------------------------------------------------------------------------------------------------------------------------------
class SegRun:
    """The buffers and the descriptor of one SegCase"""

    def __init__(self, c, tile):
        self.c = c
        lay = R.seg_layouts(c.first, c.nseg)
        self.A = [place_operand(stored_A(a, amn), amn, c.kind) for a, (amn, _) in zip(c.A, lay)]
        self.B = [place_operand(stored_B(b, bmn), bmn, c.kind) for b, (_, bmn) in zip(c.B, lay)]
        odt = torch.bfloat16 if c.out_bf16 else torch.float32
        self.C = Placed((c.nb1, c.nb2, c.M, c.N), odt, ld=_ru(c.N, 4) + 8, gaps=[4, 12], t=c.C0 if c.acc else None)
        self.D = Placed(c.D.shape, c.D.dtype, ld=_ru(c.N, 4) + 4, gaps=[4, 8], t=c.D) if c.with_d else None
        self.rs = Placed((c.nb1, c.nb2, 1, c.M), torch.float32, ld=c.M + 1, pad_rows=0, gaps=[0, 3], t=c.rs[:, :, None, :]) if c.with_d else None
        d = base_desc(M=c.M, N=c.N, K=R.SEG_K[0], nb1=c.nb1, nb2=c.nb2, alpha=c.alpha, accumulate=int(c.acc), tile=tile,
                      a_layout=int(lay[0][0]), b_layout=int(lay[0][1]), lda=self.A[0].ld, ldb=self.B[0].ld,
                      sA1=self.A[0].strides[0], sA2=self.A[0].strides[1], sB1=self.B[0].strides[0], sB2=self.B[0].strides[1],
                      sCi=self.C.ld, sC1=self.C.strides[0], sC2=self.C.strides[1])
        set_kind(d, c.kind, c.out_bf16)
        if c.with_d:
            d.base.sDi, d.base.sD1, d.base.sD2 = self.D.ld, self.D.strides[0], self.D.strides[1]
            d.base.sRS1, d.base.sRS2 = self.rs.strides[0], self.rs.strides[1]
        for i in range(1, c.nseg):
            s = d.seg[i - 1]
            s.K, s.a_layout, s.b_layout = R.SEG_K[i], int(lay[i][0]), int(lay[i][1])
            s.lda, s.ldb = self.A[i].ld, self.B[i].ld
            s.sA1, s.sA2 = self.A[i].strides[0], (0 if i >= 2 else self.A[i].strides[1])      # (shared by the groups)
            s.sB1, s.sB2 = self.B[i].strides[0], self.B[i].strides[1]
        self.d = d

    def run(self):
        return call(self.d, self.A, self.B, self.C, self.rs, self.D)

    def kernel(self, tile):
        c = self.c
        return f"gemm_{'MM' if c.first == 'MM' else 'KM'}{'+KM+MM+KM' if c.nseg > 2 else '+KM'}_{c.kind}_{tile}"


def _seg_ids():
    return [(k, fi) for k in R.KINDS for fi, (_, n) in enumerate(R.SEG_FORMS) if not (k == "f32" and n > 2)]


@pytest.mark.parametrize("kind,fi", _seg_ids())
def test_k_segments_against_fp64(kind, fi, prof):
    """two segments behind a K-major / MN-major and behind an MN / MN first segment, three and four segments; tiles 32 / 64 / 128 forced
    and auto (M = 70, N = 72: 32); fp32 / bf16 output, accumulate, row_scale * D walked over them (engine_forms_ref.seg_cases)"""
    first, nseg = R.SEG_FORMS[fi]
    cases = [(t, c) for t, c in R.seg_cases(_dev(), only_kind=kind) if (c.first, c.nseg) == (first, nseg)]
    assert len(cases) == 4
    for tile, c in cases:
        r = SegRun(c, tile)
        C0 = r.C.bits() if c.acc else None

        def fn():
            if C0 is not None:
                r.C.flat.view(_ity(r.C.dtype)).copy_(C0)
            return r.run()
        twice(fn, [r.C], c.name)
        assert prof() == {r.kernel(tile or 32)}, c.name
        margin(f"{c.name} tile {tile}", R.check_bound(r.C.view(), *c.ref(), f"{c.name} tile {tile} (frame, group, row, column)"))
        r.C.untouched_outside(c.name)


@pytest.mark.parametrize("kind,fi", _seg_ids())
def test_k_segments_same_bits_on_every_tile(kind, fi, prof):
    """gemm.hip: the result must not depend on the tile the block count picks -- M = 150, N = 136 on the 32, 64 and 128 tiles"""
    first, nseg = R.SEG_FORMS[fi]
    c = R.SegCase(kind, first, nseg, big=True, out_bf16=False, acc=False, with_d=True, device=_dev())
    got = {}
    for tile in (32, 64, 128):
        r = SegRun(c, tile)
        assert r.run() == OK, last_error()
        assert prof() == {r.kernel(tile)}
        got[tile] = r.C.bits()
    assert torch.equal(got[32], got[64]) and torch.equal(got[64], got[128]), f"{c.name}: the tiles disagree"


def test_k_segment_refusals_launch_nothing(prof):
    """the engine's own refusals through the test entry point: its status, C keeps the sentinel, nothing launched"""
    def fresh(kind="bf16", first="KM", nseg=4):
        return SegRun(R.SegCase(kind, first, nseg, device=_dev()), 0)
    ws = torch.zeros(4 * 6 * 70 * 72 + 64, device=_dev())
    lse = torch.zeros(6 * 70, device=_dev())
    cases = []
    r = fresh(nseg=3); r.A[1] = r.B[1] = None
    cases.append(("segment 3 without segment 2", r, {}, BAD_ARG))
    r = fresh(nseg=2); r.d.base.ksplit = 2
    cases.append(("a second segment with ksplit 2", r, dict(ws=ws), BAD_ARG))
    r = fresh(nseg=2); r.d.epi = 2
    cases.append(("a second segment with an epilogue", r, dict(row_lse=lse), BAD_ARG))
    r = fresh(nseg=2); r.d.nb3 = 2
    cases.append(("a second segment with nb3 = 2", r, {}, BAD_ARG))
    r = fresh(nseg=4); r.d.base.ksplit = 2
    cases.append(("four segments with ksplit 2", r, dict(ws=ws), BAD_ARG))
    r = fresh(kind="f32s3", nseg=3); r.d.base.fp32_planes = 0
    cases.append(("segment 3 in plain fp32", r, {}, BAD_ARG))
    r = fresh(nseg=3); r.d.base.a_layout = 1
    cases.append(("segment 3 behind an MN-major A", r, {}, BAD_ARG))
    r = fresh(nseg=3); r.d.base.b_layout = 0
    cases.append(("segment 3 behind a K-major B", r, {}, BAD_ARG))
    r = fresh(nseg=2); r.d.seg[0].a_layout = 1
    cases.append(("segment 2 with A MN-major", r, {}, UNSUPPORTED))
    r = fresh(kind="f32s3", nseg=2); r.d.seg[0].b_layout = 0
    cases.append(("segment 2 with B K-major", r, {}, UNSUPPORTED))
    r = fresh(nseg=3); r.d.seg[1].a_layout = 0
    cases.append(("segment 3 with A K-major", r, {}, UNSUPPORTED))
    for what, r, kw, want in cases:
        st = call(r.d, [x for x in r.A], [x for x in r.B], r.C, None, None, **kw)
        assert st == want, f"{what}: status {st}, expected {want} ({last_error()})"
        assert r.C.poisoned(), f"{what}: C was written"
        assert not prof(), f"{what}: a kernel was launched"


# ---- third batch level -----------------------------------------------------------------------------------------------------------------------
class Nb3Run:
    """the dTW pattern: C blocks interleaved in one buffer -- slot b3 at row block b3 and at column offset b3 * coff inside group b2's columns:
    sC3 = M * ld + coff, sC2 = 2 * coff rounded up to a multiple of 4, the other slot's columns and a pad row per frame keep the sentinel"""

    def __init__(self, c, ksplit=1, coff=None):
        self.c = c
        coff = c.N if coff is None else coff
        self.A = place_operand(stored_A(c.A, True), True, c.kind)
        self.B = place_operand(stored_B(c.B, True), True, c.kind)
        sC2 = _ru(coff + c.N, 4)
        ld = c.nb2 * sC2 + 8
        sC3 = c.M * ld + coff
        sC1 = (c.nb3 * c.M + 1) * ld
        odt = torch.bfloat16 if c.out_bf16 else torch.float32
        self.C = Placed((c.nb1, c.nb3, c.nb2, c.M, c.N), odt, ld=ld, strides=(sC1, sC3, sC2))
        self.ws = None
        d = base_desc(M=c.M, N=c.N, K=c.K, nb1=c.nb1, nb2=c.nb2, nb3=c.nb3, a_layout=1, b_layout=1, lda=self.A.ld, ldb=self.B.ld, ksplit=ksplit,
                      sA1=self.A.strides[0], sA3=self.A.strides[1], sA2=self.A.strides[2], sB1=self.B.strides[0], sB3=self.B.strides[1],
                      sB2=self.B.strides[2], sCi=ld, sC1=sC1, sC3=sC3, sC2=sC2)
        set_kind(d, c.kind, c.out_bf16)
        if ksplit > 1:
            self.ws = Placed((ksplit * c.nb1 * c.nb3 * c.nb2 * c.M, c.N), torch.float32, ld=c.N, pad_rows=0)
        self.d = d

    def run(self):
        return call(self.d, [self.A], [self.B], self.C, ws=self.ws)


@pytest.mark.parametrize("kind", list(R.KINDS))
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("ksplit", [1, 3])
def test_third_batch_level_against_fp64(kind, out_bf16, ksplit, prof):
    c = R.Nb3Case(kind, out_bf16, device=_dev())
    r = Nb3Run(c, ksplit)
    assert r.d.sC3 % 4 == 0
    twice(r.run, [r.C], c.name)
    assert prof() == {f"gemm_MM_{kind}_32"} | ({"gemm_splitk_reduce"} if ksplit > 1 else set()), c.name
    margin(f"{c.name} ksplit {ksplit}", R.check_bound(r.C.view(), *c.ref(), f"{c.name} ksplit {ksplit} (frame, slot, group, row, column)"))
    r.C.untouched_outside(c.name)
    if r.ws is not None:
        r.ws.untouched_outside(c.name + " slabs")


@pytest.mark.parametrize("kind", ["bf16", "f32s3"])
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("ksplit", [1, 3])
def test_sc3_off_the_vector_grid_takes_the_scalar_stores(kind, out_bf16, ksplit, prof):
    """sC3 = M * ld + 50: not a multiple of four output elements, every other C stride is -- launch_gemm must leave the 16-byte (8-byte for
    bf16) store path (vec_c looks at sC3 when nb3 > 1), and the result matches"""
    c = R.Nb3Case(kind, out_bf16, device=_dev())
    r = Nb3Run(c, ksplit, coff=50)
    assert r.d.sC3 % 4 == 2 and r.d.base.sC1 % 4 == 0 and r.d.base.sC2 % 4 == 0 and r.d.base.sCi % 4 == 0
    twice(r.run, [r.C], c.name)
    assert f"gemm_MM_{kind}_32" in prof()
    margin(f"{c.name} ksplit {ksplit} sC3 odd", R.check_bound(r.C.view(), *c.ref(), f"{c.name} sC3 = {r.d.sC3} (frame, slot, group, row, column)"))
    r.C.untouched_outside(c.name)
    same = Nb3Run(c, ksplit)                       # the vector path on the same operands: the same values
    assert same.run() == OK
    assert torch.equal(same.C.view().contiguous().view(_ity(same.C.dtype)), r.C.view().contiguous().view(_ity(r.C.dtype)))


def test_third_batch_level_refusals_launch_nothing(prof):
    c = R.Nb3Case("bf16", False, device=_dev())
    D = torch.zeros(64 * 1024, device=_dev(), dtype=torch.bfloat16)
    rs = torch.zeros(4096, device=_dev())
    r = Nb3Run(c); r.d.base.sDi = 64
    assert call(r.d, [r.A], [r.B], r.C, rs, D) == BAD_ARG, "nb3 with a D term"
    assert r.C.poisoned() and not prof()
    r = Nb3Run(c); r.d.epi = 2
    assert call(r.d, [r.A], [r.B], r.C, row_lse=rs) == BAD_ARG, "nb3 with an epilogue"
    assert r.C.poisoned() and not prof()
    r = Nb3Run(c)
    s = r.d.seg[0]
    s.K, s.a_layout, s.b_layout, s.lda, s.ldb = c.K, 0, 1, r.A.ld, r.B.ld
    assert call(r.d, [r.A, r.A], [r.B, r.B], r.C) == BAD_ARG, "nb3 with a second segment"
    assert r.C.poisoned() and not prof()


# ---- kept slabs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_kept_slabs_against_fp64(kind, prof):
    """ksplit = 4, keep_slabs: the fp64 sum of the slabs [ksplit][batch][M][N] meets the product bound; C untouched; no reduce pass"""
    c = R.SlabCase(kind, device=_dev())
    A, B = place_operand(c.A, False, kind), place_operand(c.B, True, kind)
    Cc = Placed((c.nb1, c.nb2, c.M, c.N), torch.float32, ld=c.N + 4)
    ws = Placed((c.ksplit, c.nb1, c.nb2, c.M, c.N), torch.float32, ld=c.N, pad_rows=0, gaps=[0, 0, 0])
    d = base_desc(M=c.M, N=c.N, K=c.K, nb1=c.nb1, nb2=c.nb2, a_layout=0, b_layout=1, lda=A.ld, ldb=B.ld, ksplit=c.ksplit, keep_slabs=1, tile=64,
                  sA1=A.strides[0], sA2=A.strides[1], sB1=B.strides[0], sB2=B.strides[1], sCi=Cc.ld, sC1=Cc.strides[0], sC2=Cc.strides[1])
    set_kind(d, kind, False)
    twice(lambda: call(d, [A], [B], Cc, ws=ws), [ws, Cc], c.name)
    assert prof() == {f"gemm_KM_{kind}_64"}, "a reduce scope, or another kernel"
    assert Cc.poisoned(), "C was written"
    ws.untouched_outside(c.name + " slabs")
    ref, bound = c.ref()
    margin(c.name, R.check_bound(ws.view().double().sum(0), ref, bound, f"{c.name} (frame, group, row, column)"))
    # each slab against its own K range: a slab written to another slab's place would still give the right sum
    per = c.kper()
    for s in range(c.ksplit):
        k0, k1 = min(c.K, s * per), min(c.K, (s + 1) * per)
        if k1 > k0:
            sref, smag = R.product_ref(c.A[..., k0:k1], c.B[..., k0:k1, :])
            R.check_bound(ws.view()[s], sref, R.form_bound(sref, smag, smag, kind=kind, out_bf16=False, k_terms=k1 - k0), f"{c.name} slab {s}")
        else:
            assert bool((ws.view()[s] == 0).all()), f"{c.name}: slab {s} has no K entries and is not zero"


# ---- softmax epilogues -----------------------------------------------------------------------------------------------------------------------
class SoftmaxRun:
    def __init__(self, c):
        self.c = c
        F, M, N, K = c.shape
        kind = c.kind
        self.B = place_operand(c.B, False, kind, kpad=0.0)
        if c.shared:                                # A = the first M tokens of B's buffer
            self.A = self.B
        else:
            self.A = place_operand(c.A, False, kind, kpad=7.0)
        self.odt = R.tdtype(kind)
        self.ldc = _ru(N, 4) + 4

    def desc(self, epi, alpha, D=None, **kw):
        F, M, N, K = self.c.shape
        d = base_desc(M=M, N=N, K=K, nb1=F, nb2=1, alpha=alpha, epi=epi, a_layout=0, b_layout=0, lda=self.A.ld, ldb=self.B.ld,
                      sA1=self.A.strides[0], sB1=self.B.strides[0], sCi=self.ldc, sC1=M * self.ldc + 4, **kw)
        set_kind(d, self.c.kind, self.c.kind == "bf16")
        if D is not None:
            d.base.sDi, d.base.sD1 = D.ld, D.strides[0]
        return d

    def out(self):
        F, M, N, K = self.c.shape
        return Placed((F, M, N), self.odt, ld=self.ldc, strides=(M * self.ldc + 4,))

    def kernel(self):
        return f"gemm_KK_{self.c.kind}_128"


@pytest.mark.parametrize("kind", R.SOFTMAX_KINDS)
@pytest.mark.parametrize("family,shape", R.softmax_ids())
def test_softmax_epilogues_against_fp64(kind, family, shape, prof):
    from avmoe_amd import _capi
    c = R.SoftmaxCase(kind, family, shape, device=_dev())
    run = SoftmaxRun(c)
    F, M, N, K = shape
    for alpha in (1.0, 0.5):
        r = c.at(alpha)
        name = f"{c.name} alpha {alpha}"
        # ---- ROWSTATS: every (max, sum) pair; C untouched ------------------------------------------------------------------------
        parts = Placed((F * M, 2 * c.tiles), torch.float32, ld=2 * c.tiles, pad_rows=0)
        Cc = run.out()
        d = run.desc(_capi.EPI_ROWSTATS, alpha)
        twice(lambda: call(d, [run.A], [run.B], Cc, row_part=parts), [parts, Cc], name + " ROWSTATS")
        assert prof() == {run.kernel()}, name
        assert Cc.poisoned(), f"{name}: ROWSTATS wrote C"
        parts.untouched_outside(name + " row_part")
        pk = parts.view().reshape(F, M, c.tiles, 2)
        (mr, mb), (sr, sb) = r.parts(pk[..., 0])
        margin(name + " ROWSTATS max", R.check_bound(pk[..., 0], mr, mb, name + " ROWSTATS max (frame, row, tile)"))
        margin(name + " ROWSTATS sum", R.check_bound(pk[..., 1], sr, sb, name + " ROWSTATS sum (frame, row, tile)"))
        # ---- lse of the kernel's own parts ---------------------------------------------------------------------------------------
        lse = Placed((1, F * M), torch.float32, ld=F * M, pad_rows=0)
        twice(lambda: row_lse(parts, F * M, c.tiles, lse), [lse], name + " row_lse")
        assert prof() == {"gemm_row_lse"}
        lse.untouched_outside(name + " lse")
        lk = lse.view().reshape(F, M)
        margin(name + " lse of its parts", R.check_bound(lk, *R.row_lse_ref(pk), name + " lse against its parts (frame, row)"))
        margin(name + " lse of the scores", R.check_bound(lk, r.lse_true, R.lse_from_scores_bound(pk, sr, sb), name + " lse against the scores (frame, row)"))
        # ---- EXP from a given lse with per-row offsets -----------------------------------------------------------------------------
        Cc = run.out()
        d = run.desc(_capi.EPI_EXP, alpha)
        twice(lambda: call(d, [run.A], [run.B], Cc, row_lse=r.lse_in), [Cc], name + " EXP")
        assert prof() == {run.kernel()}
        margin(name + " EXP", R.check_bound(Cc.view(), *r.exp(r.lse_in), name + " EXP (frame, row, column)"))
        Cc.untouched_outside(name + " EXP")
        # ---- MULSUB with a drawn rowdot and a drawn D: the vector and the scalar D path --------------------------------------------
        got = []
        for path, ldd in (("vector D", _ru(N, 4) + 4), ("scalar D", N + (1 if (N + 1) % 4 else 2))):
            D = Placed((F, M, N), run.odt, ld=ldd, gaps=[4 if path == "vector D" else 1], t=c.D)
            assert (ldd % 4 == 0) == (path == "vector D")
            Cc = run.out()
            d = run.desc(_capi.EPI_MULSUB, alpha, D=D)
            twice(lambda: call(d, [run.A], [run.B], Cc, D=D, row_lse=r.rowdot), [Cc], f"{name} MULSUB {path}")
            assert prof() == {run.kernel()}
            margin(f"{name} MULSUB {path}", R.check_bound(Cc.view(), *r.mulsub(r.rowdot, c.D), f"{name} MULSUB {path} (frame, row, column)"))
            Cc.untouched_outside(f"{name} MULSUB {path}")
            got.append(Cc.bits())
        assert torch.equal(got[0], got[1]), f"{name}: the vector and the scalar D path give other bits"


@pytest.mark.parametrize("what,rows,tiles", R.LSE_ALONE)
def test_row_lse_alone_on_constructed_parts(what, rows, tiles, prof):
    """one tile; a tile 150 below the row maximum, whose term underflows; 1, 257 and 1 048 579 rows (the last enters the grid-stride loop)"""
    parts = R.lse_alone_parts(what, rows, tiles, device=_dev())
    lse = Placed((1, rows), torch.float32, ld=rows, pad_rows=0)
    twice(lambda: row_lse(parts, rows, tiles, lse), [lse], what)
    assert prof() == {"gemm_row_lse"}
    margin(f"row_lse alone: {what}", R.check_bound(lse.view()[0], *R.row_lse_ref(parts), f"row_lse alone, {what} (row)"))
    lse.untouched_outside(what)


def test_row_lse_refusals_and_no_rows(prof):
    lse = Placed((1, 8), torch.float32, ld=8, pad_rows=0)
    parts = torch.zeros(8, 2, 2, device=_dev())
    assert row_lse(parts, 0, 2, lse) == OK and row_lse(None, 8, 2, lse) == BAD_ARG and row_lse(parts, 8, 2, None) == BAD_ARG
    assert row_lse(parts, 8, 0, lse) == BAD_ARG
    assert lse.poisoned() and not prof()


def test_softmax_refusals_launch_nothing(prof):
    """launch_gemm's refusals for the epilogues: ksplit, accumulate, row_scale, column-major C, a forced tile other than 128"""
    from avmoe_amd import _capi
    c = R.SoftmaxCase("bf16", "free", R.SOFTMAX_FREE[2], device=_dev())
    run = SoftmaxRun(c)
    F, M, N, K = c.shape
    lse = torch.zeros(F * M, device=_dev())
    parts = Placed((F * M, 2), torch.float32, ld=2, pad_rows=0)
    ws = torch.zeros(2 * F * M * N + 64, device=_dev())
    rs = torch.ones(F * M, device=_dev())
    cases = [("ksplit 2", dict(ksplit=2), dict(ws=ws)), ("accumulate", dict(accumulate=1), {}), ("row_scale", {}, dict(rs=rs)),
             ("column-major C", dict(sCi=1, sCj=run.ldc), {}), ("tile 64", dict(tile=64), {}), ("tile 32", dict(tile=32), {})]
    for epi in (_capi.EPI_ROWSTATS, _capi.EPI_EXP):
        for what, dk, ck in cases:
            d = run.desc(epi, 1.0)
            for k, v in dk.items():
                setattr(d.base, k, v)
            Cc = run.out()
            st = call(d, [run.A], [run.B], Cc, row_part=parts, row_lse=lse, **ck)
            assert st == BAD_ARG, f"epi {epi} with {what}: status {st} ({last_error()})"
            assert Cc.poisoned() and parts.poisoned() and not prof(), f"epi {epi} with {what}: something ran"
    d = run.desc(_capi.EPI_MULSUB, 1.0)              # MULSUB without its D, EXP without its lse
    Cc = run.out()
    assert call(d, [run.A], [run.B], Cc, row_lse=lse) == BAD_ARG and call(run.desc(_capi.EPI_EXP, 1.0), [run.A], [run.B], Cc) == BAD_ARG
    assert Cc.poisoned() and not prof()


def test_every_form_was_checked():
    """Closes the module (runs after the tests above and fails when they did not run): every type met every K-segment form on every tile,
    the third batch level with and without split-K and off the vector grid, kept slabs, and every softmax case at both alpha."""
    need = [f"segments {k} {f}x{n}" for k in R.KINDS for f, n in R.SEG_FORMS if not (k == "f32" and n > 2)]
    need += [f"nb3 {k}" for k in R.KINDS] + [f"kept slabs {k}" for k in R.KINDS] + ["sC3 odd"]
    need += [f"softmax {k} {fam} {'x'.join(map(str, s))} alpha {a} {op}" for k in R.SOFTMAX_KINDS for fam, s in R.softmax_ids() for a in (1.0, 0.5)
             for op in ("ROWSTATS max", "ROWSTATS sum", "lse of its parts", "lse of the scores", "EXP", "MULSUB vector D", "MULSUB scalar D")]
    missing = [n for n in need if not any(n in m for m in MARGINS)]
    for m, v in sorted(MARGINS.items()):
        print(f"COVERED {m} {v:.4f}")
    assert not missing, f"not checked: {missing}"
    for t in (32, 64, 128, 0):
        assert sum(f"tile {t}" in m for m in MARGINS) >= 14, f"tile {t}"
